#!/usr/bin/env python
"""Route M alone at the bench shape: whole maskgit_generate calls (18 iterations, Philox noise) of the bench model (presets.config2(6), synthetic weights) on B six-view
scenes, timed with HIP events; ms per call, scenes/s and the best of N calls.  One process per run: A/B arms alternate processes (experiments/r12.md).
usage: route_m_probe.py [B=16] [precision=f16x3|f16x1|fp32] [weights=f32|f16] [N=5] [timesteps=18]
(N = 1 and timesteps = 2 under `rocprofv3 --kernel-trace`: a short call whose launch sequence and ids two builds of the library must share, tools/launch_sequence.py)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hashlib
import torch
from bevgen_amd import presets, synthetic
from bevgen_amd.runtime import Context
from bevgen_amd.weights import maskgit_state_dict

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
precision = sys.argv[2] if len(sys.argv) > 2 else "f16x3"
weights = sys.argv[3] if len(sys.argv) > 3 else "f32"
N = int(sys.argv[4]) if len(sys.argv) > 4 else 5
timesteps = int(sys.argv[5]) if len(sys.argv) > 5 else 18
cfg = presets.config2(6)
ctx = Context(cfg, route="maskgit", max_batch=B, precision=precision, weights=weights)
ctx.load_state_dict(maskgit_state_dict(cfg, 1234))
ctx.set_tables()
ctx.finalize()
bt = {k: v.cuda() for k, v in synthetic.make_batch(cfg, B, seed=0).items()}
run = lambda seed: ctx.maskgit_generate(bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], timesteps=timesteps, noise_seed=seed, check=False)
run(2025)   # warm-up: workspace, one-time attributes
torch.cuda.synchronize()
ms = []
for i in range(N):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    ids = run(2025 + i)
    t1.record()
    t1.synchronize()
    ms.append(t0.elapsed_time(t1))
ctx.synchronize()   # (reads the status word: a raised flag fails the run)
mean = sum(ms) / len(ms)
sha = hashlib.sha256(ids.cpu().numpy().tobytes()).hexdigest()[:16]   # the last call's ids: a fingerprint for arms that must agree
print(f"B={B} precision={precision} weights={weights} timesteps={timesteps}: {mean:.2f} ms per call, {B * 1e3 / mean:.3f} scenes/s (mean of {N}); best {min(ms):.2f} ms, {B * 1e3 / min(ms):.3f} scenes/s; "
      f"calls {' '.join(f'{t:.2f}' for t in ms)}; ids sha256 {sha}")
ctx.close()
