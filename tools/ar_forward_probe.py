#!/usr/bin/env python
"""Route A teacher-forced forward on one GPU: the stepwise GPT.forward (prefill + N decode steps driven from Python) against the one-pass forward (bevgen_ar_forward).

    python tools/ar_forward_probe.py                 # every shape, each in a child process of its own under its own time limit
    python tools/ar_forward_probe.py --shape config4 --batch 16 --kv f16 [--score] [--skip-stepwise]

Per shape: median wall time of 5 forwards after 2 warm-ups (device synchronised around each), ms per forward for both paths, and for the one-pass form the rows x FLOP
per row as achieved TFLOP/s (2 x 12 D^2 multiply-adds per layer and row + the attention products over the visible keys; about 0.55 GFLOP per row at config 4).  One JSON
line per shape on stdout.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [  # (shape, batch, kv, time limit in seconds)
    ("tiny", 2, "f32", 120),
    ("config4", 1, "f32", 300),
    ("config4", 1, "f16", 300),
    ("config4", 16, "f32", 420),
    ("config4", 16, "f16", 420),
]


def timed(fn, warmup=2, reps=5):
    import torch

    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def run_shape(shape, B, kv, score, skip_stepwise, reps):
    import torch

    from bevgen_amd import presets, synthetic, weights as W
    from bevgen_amd.modules.transformer.mingpt_sparse import GPT

    cfg = presets.tiny_route_a(3, block=16) if shape == "tiny" else presets.config4()
    gpt = GPT(cfg, precision="fp32", kv_cache=kv)
    gpt.load_state_dict(W.gpt_state_dict(cfg, 1234))
    gpt = gpt.to("cuda")
    bt = synthetic.make_batch(cfg, B, seed=2)
    batch = {"intrinsics_inv": bt["intrinsics_inv"].cuda(), "extrinsics_inv": bt["extrinsics_inv"].cuda()}
    cond = bt["cond_ids"].cuda()
    ids = torch.randint(0, cfg.vocab_size, (B, cfg.num_cams, cfg.num_cam_tokens), generator=torch.Generator().manual_seed(1)).cuda()
    N, K, D, Lyr = cfg.num_img_tokens, cfg.num_cond_tokens, cfg.num_embed, cfg.num_layers
    rows = B * (K + N)
    # multiply-adds x 2: projections 12 D^2 per row and layer, attention 2 x 2 x D per visible key (causal: about half of K + N on average), head D V on the N scored rows
    flop = 2.0 * rows * Lyr * 12 * D * D + 4.0 * rows * Lyr * D * (K + N) / 2 + 2.0 * B * N * D * cfg.vocab_size
    rec = {"shape": shape, "B": B, "kv": kv, "N": N, "K": K, "rows": rows, "gflop_per_row": flop / rows / 1e9}
    if score:
        one = lambda: gpt.score(ids, cond, batch, sampling=True)
        rec["onepass_form"] = "score (no logits buffer)"
    else:
        one = lambda: gpt.forward_onepass(ids, cond, batch, sampling=True)
        rec["onepass_form"] = "logits"
    med, lo, hi = timed(one, reps=reps)
    rec.update(onepass_ms=round(med, 3), onepass_min_ms=round(lo, 3), onepass_max_ms=round(hi, 3), onepass_tflops=round(flop / med / 1e9, 2))
    if not skip_stepwise:
        med, lo, hi = timed(lambda: gpt(ids, cond, batch, sampling=True), reps=reps)
        rec.update(stepwise_ms=round(med, 3), stepwise_min_ms=round(lo, 3), stepwise_max_ms=round(hi, 3), speedup=round(med / rec["onepass_ms"], 2))
        a = gpt(ids, cond, batch, sampling=True)
        b = gpt.forward_onepass(ids, cond, batch, sampling=True)
        rec["max_abs_diff"] = float((a - b).abs().max())
        rec["max_abs_logit"] = float(a.abs().max())
    gpt.invalidate()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["tiny", "config4"])
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--kv", choices=["f32", "f16"], default="f32")
    ap.add_argument("--score", action="store_true", help="time GPT.score (nll + loss, no logits buffer) as the one-pass form")
    ap.add_argument("--skip-stepwise", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.shape:
        run_shape(a.shape, a.batch, a.kv, a.score, a.skip_stepwise, a.reps)
        return 0
    for shape, B, kv, limit in SHAPES:   # one fresh process per shape; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--batch", str(B), "--kv", kv, "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, timeout=limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"shape": shape, "B": B, "kv": kv, "error": f"time limit of {limit} s"}), flush=True)
            return 1
        if r.returncode != 0:
            print(json.dumps({"shape": shape, "B": B, "kv": kv, "error": f"exit status {r.returncode}"}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
