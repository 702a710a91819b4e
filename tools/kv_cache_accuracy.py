#!/usr/bin/env python
"""Route A: what a lossy KV-cache storage mode costs in the logits.  BASELINE config 4 (L=2368, 24 layers, synthetic weights), B sequences, `steps` decode steps,
teacher forced with the greedy tokens of the exact model (kv_cache='f32'): per mode the relative distance of every step's logits from the exact model's,
max |a - b| / max |b| per step (worst and mean over the steps), and the share of (step, sequence) pairs whose arg-max is the exact model's.
usage: kv_cache_accuracy.py [B=2] [steps=2100] [kv=f16,i8] [weights=f32]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bevgen_amd import presets, synthetic
from bevgen_amd.runtime import Context
from bevgen_amd.weights import gpt_state_dict

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2100
kvs = (sys.argv[3] if len(sys.argv) > 3 else "f16,i8").split(",")
weights = sys.argv[4] if len(sys.argv) > 4 else "f32"
cfg = presets.config4()
sd = gpt_state_dict(cfg, 1234)
bt = {k: v.cuda() for k, v in synthetic.make_batch(cfg, B, seed=0).items()}
args = (bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"])


def run(kv, forced):
    ctx = Context(cfg, route="ar", max_batch=B, kv_cache=kv, decode_path="fused", decode_weights=weights)
    ctx.load_state_dict(sd)
    ctx.set_tables()
    ctx.finalize()
    x, logits = ctx.ar_sample(*args, steps=steps, greedy=True, return_logits=True, forced_ids=forced)
    torch.cuda.synchronize()
    x, logits = x.cpu(), logits.cpu()
    ctx.close()
    return x, logits


x, ref = run("f32", None)
T = cfg.num_cam_tokens
idx = torch.as_tensor([int(j) for j in cfg.forward_shuffle_idx[:steps]])
forced = x[:, idx // T, idx % T].t().contiguous()            # [steps, B] in decode order
top2 = ref.topk(2, dim=-1).values
print(f"config 4, B={B}, steps={steps}, decode_weights={weights}: exact model's mean top-2 logit margin {float((top2[..., 0] - top2[..., 1]).mean()):.3e}, "
      f"mean max |logit| {float(ref.abs().amax(-1).mean()):.3e}", flush=True)
for kv in kvs:
    _, lg = run(kv, forced.cuda())
    d = (lg - ref).abs().amax((1, 2)) / ref.abs().amax((1, 2)).clamp_min(1e-30)
    agree = (lg.argmax(-1) == ref.argmax(-1)).float().mean().item()
    print(f"kv={kv}: relative logit distance per step worst {d.max().item():.3e} mean {d.mean().item():.3e} (last 100 steps mean {d[-100:].mean().item():.3e}); "
          f"greedy-token agreement {agree:.4f}", flush=True)
