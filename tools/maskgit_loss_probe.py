#!/usr/bin/env python
"""Cost of MaskGit.forward's loss tail on one GPU: one bevgen_maskgit_loss call (mask, forward with logits, masked cross-entropy, gumbel pick, forward with the embedding
only, critic BCE) against the two bare bevgen_muse_forward calls it contains, one with logits and one with the embedding only.

    python tools/maskgit_loss_probe.py [--batch 16] [--precision f16x3] [--reps 10]     # BASELINE config 2 (6 views of 256 x 256), one JSON line on stdout
    python tools/maskgit_loss_probe.py --profile                                        # three loss calls and nothing else: the run to put under rocprofv3 --kernel-trace

The three calls are timed in the same process, alternating (loss, logits forward, embed forward) x reps after 3 warm-ups of each, with device events around each call; the
line carries the median, minimum and maximum of each and the tail = loss - (logits forward + embed forward)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tiny", action="store_true", help="the tiny fixture shape instead of config 2 (a rehearsal of the script, not a measurement)")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import torch

    from bevgen_amd import presets, synthetic, weights as W
    from bevgen_amd.runtime import Context

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to measure without one"
    cfg = presets.tiny_route_m(3, legacy=False) if a.tiny else presets.config2(6)
    B = a.batch
    ctx = Context(cfg, route="maskgit", precision=a.precision, max_batch=B)
    ctx.load_state_dict(W.maskgit_state_dict(cfg, 1234))
    ctx.set_tables()
    ctx.finalize()
    bt = {k: v.cuda() for k, v in synthetic.make_batch(cfg, B, seed=2).items()}
    rows, T, V = B * cfg.num_cams, cfg.num_cam_tokens, cfg.vocab_size
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, V, (rows, T), generator=g).cuda()
    n = (T * torch.cos(torch.rand(rows, generator=g) * torch.pi * 0.5)).round().clamp(min=1).long().tolist()
    x = torch.where(torch.rand(rows, T, generator=g).cuda() < 0.5, torch.full_like(ids, V), ids)
    geo = (bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"])

    calls = {
        "loss": lambda: ctx.maskgit_loss(ids, *geo, n, temperature=0.7, noise_seed=77, check=False),
        "forward_logits": lambda: ctx.muse_forward(x, *geo, want_logits=True, want_embed=False, check=False),
        "forward_embed": lambda: ctx.muse_forward(x, *geo, want_logits=False, want_embed=True, check=False),
    }
    if a.profile:
        for _ in range(3):
            calls["loss"]()
        ctx.synchronize()
        print(json.dumps({"profile": "3 x maskgit_loss", "batch": B, "precision": a.precision, "masked": sum(n), "positions": rows * T}))
        return
    for fn in calls.values():
        for _ in range(3):
            fn()
    ctx.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    ctx.synchronize()
    med = {k: statistics.median(v) for k, v in ms.items()}
    tail = med["loss"] - med["forward_logits"] - med["forward_embed"]
    out = {"shape": "tiny" if a.tiny else "config2_6cam", "batch": B, "precision": a.precision, "reps": a.reps, "masked": sum(n), "positions": rows * T,
           **{k + "_ms": {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()},
           "tail_ms": round(tail, 4), "tail_share_of_two_forwards": round(tail / (med["forward_logits"] + med["forward_embed"]), 5)}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
