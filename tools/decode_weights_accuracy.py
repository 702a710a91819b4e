#!/usr/bin/env python
"""Route A: what a lossy decode-weight storage mode costs in the logits, alone and on top of a lossy KV cache (the weights axis next to tools/kv_cache_accuracy.py).
BASELINE config 4 (L=2368, 24 layers, synthetic weights), B sequences, `steps` decode steps, teacher forced with the greedy tokens of the exact model
(decode_weights='f32', kv_cache='f32'): per (weights, kv) pair the relative distance of every step's logits from the exact model's, max |a - b| / max |b| per step
(worst, mean, mean of the last 100 steps), and the share of (step, sequence) pairs whose arg-max is the exact model's.
usage: decode_weights_accuracy.py [B=2] [steps=2100] [weights=f16,i8] [kv=f16,i8]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bevgen_amd import presets, synthetic
from bevgen_amd.runtime import Context
from bevgen_amd.weights import gpt_state_dict

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2100
wts = (sys.argv[3] if len(sys.argv) > 3 else "f16,i8").split(",")
kvs = (sys.argv[4] if len(sys.argv) > 4 else "f16,i8").split(",")
cfg = presets.config4()
sd = gpt_state_dict(cfg, 1234)
bt = {k: v.cuda() for k, v in synthetic.make_batch(cfg, B, seed=0).items()}
args = (bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"])


def run(wt, kv, forced):
    ctx = Context(cfg, route="ar", max_batch=B, kv_cache=kv, decode_path="fused", decode_weights=wt)
    ctx.load_state_dict({k: v.clone() for k, v in sd.items()})   # (finalize rewrites the device copies only; the clone keeps that obvious)
    ctx.set_tables()
    ctx.finalize()
    x, logits = ctx.ar_sample(*args, steps=steps, greedy=True, return_logits=True, forced_ids=forced)
    torch.cuda.synchronize()
    x, logits = x.cpu(), logits.cpu()
    ctx.close()
    return x, logits


x, ref = run("f32", "f32", None)
T = cfg.num_cam_tokens
idx = torch.as_tensor([int(j) for j in cfg.forward_shuffle_idx[:steps]])
forced = x[:, idx // T, idx % T].t().contiguous()            # [steps, B] in decode order
top2 = ref.topk(2, dim=-1).values
print(f"config 4, B={B}, steps={steps}: exact model's mean top-2 logit margin {float((top2[..., 0] - top2[..., 1]).mean()):.3e}, "
      f"mean max |logit| {float(ref.abs().amax(-1).mean()):.3e}", flush=True)
for wt in wts:
    for kv in ["f32"] + kvs:
        _, lg = run(wt, kv, forced.cuda())
        d = (lg - ref).abs().amax((1, 2)) / ref.abs().amax((1, 2)).clamp_min(1e-30)
        agree = (lg.argmax(-1) == ref.argmax(-1)).float().mean().item()
        print(f"weights={wt} kv={kv}: relative logit distance per step worst {d.max().item():.3e} mean {d.mean().item():.3e} (last 100 steps mean {d[-100:].mean().item():.3e}); "
              f"greedy-token agreement {agree:.4f}", flush=True)
