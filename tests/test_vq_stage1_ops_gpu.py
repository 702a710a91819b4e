"""Operator-level parity of the two stage-1 kernels behind bevgen_vq_encode_ex (bevgen_amd/csrc/vqenc_kernels.hip), through bevgen_op_vq_geo_embed and
bevgen_op_vq_quant_error, on the fp32 and the f16x3 context (the kernels are fp32 in both).  Cases, references and e_cpu: tests/test_vq_stage1_cpu.py.

Every output sits in a sentinel-filled buffer with a guard region on both sides (tests/test_frontend_ops_gpu.py Guarded).

Bounded, bound = 4 x e_cpu (the fp32 torch evaluation's own error against fp64, recomputed where the tests run); worst error measured on an MI355X beside it (each test
prints its own, `pytest -s`):
  kernel                                    metric                                   e_cpu     bound     measured
  vq_geo_embed                              per row max |out - ref64| / max |ref64|  5.2e-8    2.1e-7    5.2e-8
  vq_quant_error, row_err (float cases)     per row |out - ref64| / ref64            2.0e-7    8.0e-7    1.3e-7
  vq_quant_error, loss (float cases)        relative; bound = the row bound + 2^-24 (a mean with positive weights of the rows, accumulated in double, rounded once):
                                                                                     -         8.5e-7    4.3e-8
Exact: integer-valued z and codebook (row_err and loss bit for bit), Wimg = Wcam = 0 (h unchanged bit for bit), two runs of either kernel, the neighbours of a NaN row.
"""
import numpy as np
import pytest
import torch

from test_frontend_ops_gpu import Guarded, dev, same_bits
from test_frontend_ref_cpu import row_err as row_rel
from test_vq_stage1_cpu import BETA, GEO_SHAPES, GPU_FACTOR, QERR_SHAPES, e_cpu, fixed_order_loss, geo_case, geo_ref, qerr_case, qerr_ref, rel_rows

pytestmark = pytest.mark.gpu

_E = {}


def bound(kernel):
    if not _E:
        _E.update(e_cpu())
    return GPU_FACTOR * _E[kernel]


@pytest.fixture(scope="module")
def gpu_ctx_split():
    from bevgen_amd.runtime import Context

    ctx = Context(None, precision="f16x3")
    yield ctx
    ctx.close()


@pytest.fixture(params=["fp32", "f16x3"])
def any_ctx(request, gpu_ctx, gpu_ctx_split):
    return gpu_ctx if request.param == "fp32" else gpu_ctx_split


def run_geo(ctx, p):
    out = Guarded(tuple(p["h"].shape))
    out.view.copy_(p["h"].cuda())
    ctx.op_vq_geo_embed(out.view, dev(p["I_inv"]), dev(p["E_inv"]), dev(p["plane"]), dev(p["Wimg"]), dev(p["Wcam"]))
    return out.host()


@pytest.mark.parametrize("shape", GEO_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vq_geo_embed(any_ctx, shape):
    p = geo_case(*shape)
    out, again = run_geo(any_ctx, p), run_geo(any_ctx, p)
    assert same_bits(out, again)
    err = row_rel(out, geo_ref(p, torch.float64))
    print(f"vq_geo_embed {shape}: {err:.2e} (bound {bound('geo'):.2e})")
    assert bool(out.isfinite().all()) and err < bound("geo")
    assert ((out.double() - p["h"].double()).norm(dim=-1) - 1).abs().max() < 1e-5       # a unit vector was added (to h of a few units: the add rounds at 2^-23)
    assert any_ctx.status() == 0


@pytest.mark.parametrize("shape", GEO_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vq_geo_embed_zero_weights_leave_h_unchanged(gpu_ctx, shape):
    p = geo_case(*shape, zero_w=True)
    assert same_bits(run_geo(gpu_ctx, p), p["h"])


def test_vq_geo_embed_refuses_other_widths(gpu_ctx):
    from bevgen_amd import _lib

    p = geo_case(1, 2, 64)
    for D in (48, 2048):
        h = torch.zeros(1, 2, D, device="cuda")
        with pytest.raises(_lib.BevgenError, match="multiple of 32"):
            gpu_ctx.op_vq_geo_embed(h, dev(p["I_inv"]), dev(p["E_inv"]), dev(p["plane"]), torch.zeros(D, 4, device="cuda"), torch.zeros(D, 4, device="cuda"))


def run_qerr(ctx, p, want_loss=True):
    """op_vq_quant_error with the row errors in a guarded buffer"""
    from bevgen_amd.runtime import _ptr

    rows, D = p["z"].shape
    out = Guarded((rows,))
    loss = Guarded((1,)) if want_loss else None
    z, cb, ids = dev(p["z"]), dev(p["codebook"]), dev(p["ids"])         # (named: they must outlive the call)
    ctx._check(ctx.lib.bevgen_op_vq_quant_error(ctx._h, _ptr(z), _ptr(cb), _ptr(ids), float(BETA), _ptr(out.view), _ptr(loss.view) if want_loss else None, rows,
                                                cb.shape[0], D, ctx._s()))
    return out.host(), (loss.host()[0] if want_loss else None)


@pytest.mark.parametrize("shape", QERR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vq_quant_error_integers_are_exact(any_ctx, shape):
    p = qerr_case(*shape, integer=True)
    row, loss = run_qerr(any_ctx, p)
    want, _ = qerr_ref(p, torch.float64)
    assert torch.equal(row.double(), want)
    assert same_bits(loss.reshape(1), torch.from_numpy(np.array([fixed_order_loss(want.numpy(), shape[2])])))
    # the wrapper: same numbers, loss optional
    r2, l2 = any_ctx.op_vq_quant_error(dev(p["z"]), dev(p["codebook"]), dev(p["ids"]), beta=BETA)
    assert same_bits(r2.cpu(), row) and l2.dim() == 0 and same_bits(l2.cpu().reshape(1), loss.reshape(1))
    r3, l3 = any_ctx.op_vq_quant_error(dev(p["z"]), dev(p["codebook"]), dev(p["ids"]), want_loss=False)
    assert l3 is None and same_bits(r3.cpu(), row)
    assert any_ctx.status() == 0


@pytest.mark.parametrize("shape", QERR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vq_quant_error_floats(any_ctx, shape):
    p = qerr_case(*shape, integer=False)
    (row, loss), (row2, loss2) = run_qerr(any_ctx, p), run_qerr(any_ctx, p)
    assert same_bits(row, row2) and same_bits(loss.reshape(1), loss2.reshape(1))
    want_row, want_loss = qerr_ref(p, torch.float64)
    e_row, e_loss = rel_rows(row, want_row), abs(float(loss) - float(want_loss)) / float(want_loss)
    print(f"vq_quant_error {shape}: row_err {e_row:.2e} (bound {bound('qerr'):.2e}), loss {e_loss:.2e} (bound {bound('qerr') + 2.0 ** -24:.2e})")
    assert e_row < bound("qerr") and e_loss < bound("qerr") + 2.0 ** -24
    # the loss is the fixed-order sum of the rows the kernel wrote
    assert same_bits(loss.reshape(1), torch.from_numpy(np.array([fixed_order_loss(row.numpy(), shape[2])])))
    # loss == NULL is accepted and changes nothing
    row3, none = run_qerr(any_ctx, p, want_loss=False)
    assert none is None and same_bits(row3, row)
    assert any_ctx.status() == 0


def test_vq_quant_error_nan_row_stays_in_its_row(gpu_ctx):
    shape = QERR_SHAPES[1]
    p = qerr_case(*shape, integer=False)
    clean, _ = run_qerr(gpu_ctx, p)
    q = dict(p, z=p["z"].clone())
    q["z"][5, 17] = float("nan")
    q["z"][70, 0] = float("inf")
    row, loss = run_qerr(gpu_ctx, q)
    assert bool(row[5].isnan()) and bool(row[70].isinf()) and bool(loss.isnan())
    keep = torch.ones(shape[0], dtype=torch.bool)
    keep[[5, 70]] = False
    assert same_bits(row[keep], clean[keep])
    assert gpu_ctx.status() == 0                   # no new status bit: in the model the arg-min in front of it has flagged such a row
