#!/usr/bin/env python
"""VQGAN decode (or encode) alone at the bench shape: n images (default 96 = 16 six-view scenes) of 16 x 16 latents -> 256 x 256 uint8 (encode: 256 x 256 fp32 images -> 16 x 16
ids); ms per scene over a few repetitions.
usage: vq_probe.py [n=96] [precision=f16x3] [reps=5] [what=decode|encode]     """
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hashlib
import torch
from bevgen_amd import presets
from bevgen_amd.runtime import Context
from bevgen_amd.weights import vq_state_dict

n = int(sys.argv[1]) if len(sys.argv) > 1 else 96
precision = sys.argv[2] if len(sys.argv) > 2 else "f16x3"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
what = sys.argv[4] if len(sys.argv) > 4 else "decode"
assert what in ("decode", "encode"), what
dd = presets.VQ_DDCONFIG_F16
ctx = Context(None, vq_ddconfig=dd, vq_n_embed=1024, vq_embed_dim=256, precision=precision)
ctx.load_state_dict(vq_state_dict(dd, 1024, 256, 99, with_encoder=what == "encode"), prefix="first_stage_model.")
ctx.finalize()
gen = torch.Generator(device="cuda").manual_seed(0)
if what == "encode":
    arg = torch.randn((n, 3, 256, 256), device="cuda", generator=gen)
    run = lambda: ctx.vq_encode(arg)
else:
    arg = torch.randint(0, 1024, (n, 256), device="cuda", generator=gen)
    run = lambda: ctx.vq_decode(arg, uint8=True)
run()
torch.cuda.synchronize()
ts = []
for _ in range(reps):
    t0 = time.time()
    out = run()
    torch.cuda.synchronize()
    ts.append(time.time() - t0)
exps = ctx.vq_range_exponents().tolist()   # of the last timed call (precision f16x3r; else empty)
head = f"n={n} precision={precision} {what}: {min(ts) * 1e3 / (n / 6):.3f} ms per six-view scene (best of {reps}; mean {sum(ts) / len(ts) * 1e3 / (n / 6):.3f})"
if what == "encode":   # the ids are the fingerprint for A/B runs over kernel variants that must not change results
    print(f"{head}, ids sha256 {hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]}, range exponents {exps}")
else:
    pix = ctx.vq_decode(arg[:12], uint8=False)   # fp32 pixels of two scenes: a bit-level fingerprint for A/B runs over kernel variants that must not change results
    sha = hashlib.sha256(pix.cpu().numpy().tobytes()).hexdigest()[:16]
    print(f"{head}, checksum {int(out.long().sum())}, fp32 pixels sha256 {sha}, range exponents {exps}")
ctx.close()
