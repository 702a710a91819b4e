"""precision='f16x1' on the GPU: Route M's projections as f16(A) f16(W)^T with fp32 accumulation - one MFMA per product where 'f16x3' issues three and weights='f16' two.

1. operator: bevgen_op_gemm codes 7 (LDS-DMA kernel), 8 (7 with the k range in three slices) and 9 (gemm_split_kernel), bias + GELU + residual, against the fp64 evaluation
   of the ROUNDED operands.  Only fp32 accumulation separates kernel and reference, so the bound is the 2e-6 (relative Frobenius) tests/test_ops_gpu.py uses for these
   kernels; the same output lies further than 1e-4 from the reference on the unrounded activation (tests/test_single_product_cpu.py, precondition (a): 1.8e-4), which a
   kernel that still multiplied a's low plane would meet to 2e-6 instead.
2. skipping equals multiplying by zero: on operands that are f16-representable the dropped products are exact zeros added to a separate accumulator, so code 7 gives
   the bits of code 4 and code 8 those of code 5.
3. model, forward: the GPU logits / embed lie 0.5 .. 2 d_mode from the rounded-weights oracle, d_mode being the distance of the oracle's single-product emulation from it,
   and nearer the emulation than that oracle.  A library that ran two or three products would sit at ~1e-6 of the oracle and fail both.
4. model, generate: valid ids, a clean status word, run-to-run identical.
5. nothing else moved: the two-product mode's bits before and after (and beside) a single-product context; VQGAN and Route A under 'f16x1' give the bits of 'f16x3'.

Measured on an MI355X: see experiments/r12.md."""
import threading

import pytest
import torch

import single_product_common as SP
from oracle import cases, restate as R

pytestmark = pytest.mark.gpu

BOUND = 2e-6          # tests/test_ops_gpu.py's bound for the split-precision GEMM kernels
FAR = 1e-4            # precondition (a)


def _op(ctx, inputs, mode):
    from bevgen_amd.runtime import _ptr, _stream

    a, w, b, r = (t.cuda().contiguous() for t in inputs)
    M, K = a.shape
    N = w.shape[0]
    out = torch.full((M, N), float("nan"), device="cuda")
    ctx._check(ctx.lib.bevgen_op_gemm(ctx._h, _ptr(a), _ptr(w), _ptr(b), _ptr(r), _ptr(out), M, N, K, 1, mode, _stream()))
    return out.cpu()


# ================================================================================================ 1. operator against fp64 on rounded operands
@pytest.mark.parametrize("shape,mode", [(s, m) for s, modes in SP.OP_CASES for m in modes])
def test_single_product_gemm_fp64_parity(gpu_ctx, shape, mode):
    o = _op(gpu_ctx, SP.op_inputs(*shape), mode)
    rounded, unrounded = SP.op_references(*shape)
    err, far = SP.rel_fro(o, rounded), SP.rel_fro(o, unrounded)
    print(f"single_product_gemm M,N,K={shape} mode={mode}: rel_fro vs rounded operands {err:.3e}, vs unrounded a {far:.3e}")
    assert err < BOUND, (shape, mode, err)          # (a NaN left by an element no launch wrote fails here too)
    assert far > FAR, (shape, mode, far)


# ================================================================================================ 2. skipping equals multiplying by zero
@pytest.mark.parametrize("shape,single,full", [((200, 136, 160), 7, 4), ((8485, 1024, 128), 7, 4), ((333, 264, 192), 8, 5)])   # (split-K: the shortest K three slices accept)
def test_single_product_gemm_equals_full_product_on_f16_operands(gpu_ctx, shape, single, full):
    inputs = SP.op_inputs(*shape, f16_exact=True)
    a, b = _op(gpu_ctx, inputs, single), _op(gpu_ctx, inputs, full)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), (shape, single, full, float((a - b).abs().max()))


# ================================================================================================ 3. model level, forward
def _ctx(cfg, sd, **kw):
    from bevgen_amd.runtime import Context

    ctx = Context(cfg, route="maskgit", **kw)
    ctx.load_state_dict(sd)            # the UNROUNDED weights: rounding is the library's job
    ctx.set_tables()
    ctx.finalize()
    return ctx


@pytest.mark.parametrize("name", SP.MODEL_CASES)
def test_single_product_forward_sits_at_the_modes_distance(name, monkeypatch):
    cfg, sd, _, bt, ids_in = SP.model_case(name)
    ctx = _ctx(cfg, sd, precision="f16x1")
    assert ctx.precision == "f16x1"
    lg, eg = (t.cpu() for t in ctx.muse_forward(ids_in, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"]))
    assert ctx.status() == 0
    ctx.close()
    for what, g, r, e in zip(("logits", "embed"), (lg, eg), SP.oracle_forward(name, monkeypatch), SP.oracle_forward(name, monkeypatch, torch.float32)):
        d_mode, d_r, d_e = SP.rel_fro(e, r), SP.rel_fro(g, r), SP.rel_fro(g, e)
        print(f"single_product_forward {name} {what}: d_mode = rel(le, lr) = {d_mode:.3e}, rel(lg, lr) = {d_r:.3e}, rel(lg, le) = {d_e:.3e}")
        assert 0.5 * d_mode <= d_r <= 2.0 * d_mode, (name, what, d_r, d_mode)
        assert d_e < d_r, (name, what, d_e, d_r)


# ================================================================================================ 4. model level, generate
def test_single_product_generate_is_valid_and_repeatable():
    name = "m_tiny_rays"
    case = cases.CASES[name]
    cfg, sd, sdr, bt, _ = SP.model_case(name)
    ctx = _ctx(cfg, sd, precision="f16x1")
    args = (bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"])
    kw = dict(depth=cfg.num_layers, heads=cfg.num_heads, timesteps=case.timesteps)
    rows, T, V, ts = case.batch * cfg.num_cams, cfg.num_cam_tokens, cfg.vocab_size, case.timesteps
    for seed in (0, 7):
        a = ctx.maskgit_generate(*args, timesteps=ts, noise_seed=seed).cpu()
        b = ctx.maskgit_generate(*args, timesteps=ts, noise_seed=seed).cpu()
        assert ctx.status() == 0
        assert int(a.min()) >= 0 and int(a.max()) < V, (seed, int(a.min()), int(a.max()))
        assert torch.equal(a, b), seed
        noise = None
        if seed:   # the uniforms the seeded call drew, written out for the oracle
            noise = {"gumbel_u": torch.stack([ctx.philox_uniform(seed, it, 0, rows * T * V, V=V) for it in range(ts)]).reshape(ts, rows, T, V).cpu(),
                     "critic_u": torch.stack([ctx.philox_uniform(seed, it, 1, rows * T) for it in range(ts)]).reshape(ts, rows, T).cpu()}
        ref = R.maskgit_generate(sdr, cfg, *args, noise=noise, **kw)
        print(f"single_product_generate {name} noise_seed={seed}: {float((a.reshape(ref.shape) == ref).float().mean()):.4f} of the tokens equal the rounded-weights oracle's")
    ctx.close()


# ================================================================================================ 5. nothing else moved
def test_two_product_mode_keeps_its_bits_around_a_single_product_context():
    """The single-product flag travels per host thread beside the split table: it must not outlive the call that set it, nor be seen by another thread's context."""
    cfg, sd, _, bt, ids_in = SP.model_case("m_tiny_rays")
    args = (ids_in, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"])
    two = _ctx(cfg, sd, precision="f16x3", weights="f16")
    before = [t.cpu() for t in two.muse_forward(*args)]
    one = _ctx(cfg, sd, precision="f16x1")
    solo = [t.cpu() for t in one.muse_forward(*args)]
    one.maskgit_generate(*args[1:], timesteps=2)
    assert not torch.equal(solo[0], before[0])                                   # (the two contexts do differ)
    after = [t.cpu() for t in two.muse_forward(*args)]                           # ... with the single-product context still alive
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    # side by side on two host threads, each on a stream of its own
    res, errs = {}, []

    def work(key, ctx):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                res[key] = [[t.cpu() for t in ctx.muse_forward(*args)] for _ in range(3)]
        except Exception as e:   # noqa: BLE001 - reported by the main thread
            errs.append((key, repr(e)))

    th = threading.Thread(target=work, args=("one", one))
    th.start()
    work("two", two)
    th.join()
    assert not errs, errs
    assert all(torch.equal(r[0], before[0]) and torch.equal(r[1], before[1]) for r in res["two"])
    assert all(torch.equal(r[0], solo[0]) and torch.equal(r[1], solo[1]) for r in res["one"])
    one.close()
    closed = [t.cpu() for t in two.muse_forward(*args)]                          # ... and after it is gone
    assert torch.equal(closed[0], before[0]) and torch.equal(closed[1], before[1])
    two.close()


def test_vqgan_under_f16x1_is_f16x3():
    from bevgen_amd.runtime import Context

    v = cases.VQ_TINY
    sdv = cases.vq_state_dict(v["dd"], v["n_embed"], v["embed_dim"], v["seed"])
    lat = v["dd"]["resolution"] // 2 ** (len(v["dd"]["ch_mult"]) - 1)
    ids = torch.randint(0, v["n_embed"], (v["n_images"], lat * lat), generator=torch.Generator().manual_seed(3))
    px = {}
    for precision in ("f16x3", "f16x1"):
        ctx = Context(None, vq_ddconfig=v["dd"], vq_n_embed=v["n_embed"], vq_embed_dim=v["embed_dim"], precision=precision)
        ctx.load_state_dict(sdv, prefix="first_stage_model.")
        ctx.finalize()
        px[precision] = ctx.vq_decode(ids, denormalize=True).cpu()
        ctx.close()
    assert torch.isfinite(px["f16x1"]).all() and torch.equal(px["f16x1"], px["f16x3"])


def test_route_a_under_f16x1_is_f16x3():
    from bevgen_amd.runtime import Context

    case = cases.CASES["a_tiny_blk16"]
    cfg = case.make_cfg()
    sd = cases.gpt_state_dict(cfg, case.weight_seed)
    bt = cases.inputs(case, cfg)
    tok = {}
    for precision in ("f16x3", "f16x1"):
        ctx = Context(cfg, route="ar", precision=precision)
        ctx.load_state_dict(sd)
        ctx.set_tables()
        ctx.finalize()
        tok[precision] = ctx.ar_sample(bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], greedy=True).cpu()
        ctx.close()
    assert torch.equal(tok["f16x1"], tok["f16x3"])
