"""The LDS-DMA GEMM's k loop on v_mfma_f32_16x16x32_f16 (BEVGEN_GEMM_MFMA16, gemm_split_glds.hip) and the layout conversion in front of its epilogues, through
bevgen_op_gemm: bias + GELU + residual against the fp64 product, the output starting as NaN so that an element no launch wrote shows.

Modes: 3 the LDS-DMA kernel, 4 the same with f16-representable weights (the low-plane product skipped), 5 its k range cut into three slices, 6 its stream-K form.
Shapes: one k-tile; fewer, as many and more k-tiles than ring stages (the four-stage ring of the small-problem block under modes 3 / 4, the three-stage ring of the 256-row
block under mode 6); ragged M and N; the throughput block with a ragged last block and a row split; the 43-column-tile width; stream-K with two launches giving the same
bits; three-slice split-K.

The bound is the relative Frobenius error 2e-6 that tests/test_ops_gpu.py uses for these kernels.  A k-tile is now one 32-deep product per instruction instead of two
16-deep ones, so the fp32 association changes and the results differ from the 32x32x16 build's in the last bits: both are rounding-level, a mis-indexed fragment or
conversion gives an error of order 1.  Worst error over the cases below, measured on an MI355X: 3.043e-07 for the 32x32x16 build (the parent commit) and 3.043e-07 for the 16x16x32 build, both at (1536, 1024, 2752) in mode 3 - the
split of the operands into f16 planes dominates, the case figures of the two builds agree to three digits.  The 16x16x32 build must stay within 1.5 x the
32x32x16 build's worst.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = 2e-6
WORST_32X32X16 = 3.043e-07   # measured with the parent commit's library on the cases below

CASES = [
    # (M, N, K), modes
    ((128, 128, 32), (3, 4, 6)),
    ((200, 136, 64), (3, 4, 6)),
    ((200, 136, 96), (3, 4, 6)),
    ((200, 136, 128), (3, 4, 6)),
    ((200, 136, 160), (3, 4, 6)),
    ((333, 264, 96), (3, 4, 6)),
    ((8485, 1024, 128), (3, 4)),
    ((3072, 5504, 64), (3, 4)),
    ((1536, 3072, 1024), (6, 3)),
    ((1536, 1024, 2752), (5, 3, 4)),
]


@functools.lru_cache(maxsize=None)
def _problem(M, N, K, f16_weights):
    """Inputs on the device and the fp64 reference, made once per (shape, weight form) and left unchanged."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g) * 3.0
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    if f16_weights:
        w = w.half().float()
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    ref = F.gelu(a.double() @ w.double().t() + b.double()) + r.double()
    return tuple(t.cuda().contiguous() for t in (a, w, b, r)), ref, float(ref.norm())


def _run(ctx, M, N, K, mode):
    from bevgen_amd.runtime import _ptr, _stream

    (da, dw, db, dr), ref, ref_norm = _problem(M, N, K, mode == 4)
    out = torch.full((M, N), float("nan"), device="cuda")
    ctx._check(ctx.lib.bevgen_op_gemm(ctx._h, _ptr(da), _ptr(dw), _ptr(db), _ptr(dr), _ptr(out), M, N, K, 1, mode, _stream()))
    o = out.cpu()
    return o, float((o.double() - ref).norm()) / ref_norm


@pytest.mark.parametrize("shape,mode", [(s, m) for s, modes in CASES for m in modes])
def test_gemm_mfma_shape_fp64_parity(gpu_ctx, shape, mode):
    M, N, K = shape
    o, err = _run(gpu_ctx, M, N, K, mode)
    print(f"gemm_mfma_shape M={M} N={N} K={K} mode={mode} rel_fro_err={err:.3e}")
    assert err < BOUND, (shape, mode, err)
    assert err <= 1.5 * WORST_32X32X16, (shape, mode, err, WORST_32X32X16)


def test_gemm_mfma_shape_stream_k_run_to_run(gpu_ctx):
    """Two stream-K launches of one problem: partial sums are added in a fixed order, in the 16x16 layout, so the bits agree."""
    M, N, K = 1536, 3072, 1024
    o1, e1 = _run(gpu_ctx, M, N, K, 6)
    o2, _ = _run(gpu_ctx, M, N, K, 6)
    gpu_ctx.synchronize()
    assert e1 < BOUND, e1
    assert torch.equal(o1, o2)
