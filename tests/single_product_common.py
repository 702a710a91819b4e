"""Shared by tests/test_single_product_cpu.py and tests/test_single_product_gpu.py: the operator problems of the single-product GEMM tests, the CPU emulation of the
mode at model level, and the distance both files measure with.  No test in here."""
import functools
import math
import types

import torch
import torch.nn.functional as F

# (M, N, K) -> the bevgen_op_gemm codes the GPU test runs it under: 7 = the LDS-DMA kernel single-product, 8 = 7 with the k range in three slices,
# 9 = gemm_split_kernel single-product
OP_CASES = [
    ((128, 128, 32), (7, 9)),        # one k-tile
    ((200, 136, 160), (7, 9)),       # ragged; more k-tiles than ring stages
    ((333, 264, 96), (7,)),          # ragged in M and N, fewer k-tiles than ring stages
    ((333, 264, 192), (8,)),         # split-K at its shortest: the launcher asks for two k-tiles per slice, so three slices need K >= 192 (K = 96 is refused, for codes 5 and 8 alike)
    ((8485, 1024, 128), (7,)),       # the 256-row throughput block, ragged last block, row split
    ((1536, 1024, 2752), (8,)),      # split-K at long K
]


def rel_fro(a, b):
    """relative Frobenius distance of a from b, in fp64"""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


@functools.lru_cache(maxsize=None)
def op_inputs(M, N, K, f16_exact=False):
    """a, w, bias, residual on the CPU, made as tests/test_gemm_mfma_shape_gpu.py::_problem makes them, w NOT rounded.  f16_exact: a and w rounded to f16-representable
    values (the operands whose low planes are exact zeros).  Made once per shape and left unchanged."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g) * 3.0
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    if f16_exact:
        a, w = a.half().float(), w.half().float()
    return a, w, b, r


@functools.lru_cache(maxsize=None)
def op_references(M, N, K):
    """fp64: gelu(f16(a) f16(w)^T + b) + r, what the single-product kernels compute up to fp32 accumulation, and the same with `a` unrounded"""
    a, w, b, r = op_inputs(M, N, K)
    wd = w.half().double().t()
    rounded = F.gelu(a.half().double() @ wd + b.double()) + r.double()
    unrounded = F.gelu(a.double() @ wd + b.double()) + r.double()
    return rounded, unrounded


def round_gemm_weights_route_m(sd):
    """The model whose Route M GEMM matrices (to_q / to_kv / to_out, the two feed-forward matrices, to_logits) are f16-representable: what weights='f16' and
    precision='f16x1' make of a state dict at finalize (tests/test_models_gpu.py::_round_gemm_weights_route_m)."""
    out = dict(sd)
    for k, v in sd.items():
        if k.endswith(("to_q.weight", "to_kv.weight", "to_out.weight", "to_logits.weight")) or (".transformer_blocks.layers." in k and k.endswith((".2.1.weight", ".2.4.weight"))):
            out[k] = v.half().to(v.dtype)
    return out


def single_product_functional(products=torch.float32):
    """torch.nn.functional with a `linear` that rounds input and weight to f16 and multiplies and accumulates them in `products` (fp32 as the kernels do, or fp64: the
    same projections without accumulation error; the rest of the model stays fp32 either way): the single-product projection.  For
    monkeypatch.setattr(oracle.restate, "F", ...)."""

    def linear(x, w, b=None):
        return F.linear(x.half().to(products), w.half().to(products), None if b is None else b.to(products)).to(x.dtype)

    proxy = types.SimpleNamespace(**{k: getattr(F, k) for k in dir(F) if not k.startswith("__")})
    proxy.linear = linear
    return proxy


MODEL_CASES = ("m_tiny_rays", "m_tiny_6cam")
_model_cache = {}


def model_case(name):
    """(cfg, unrounded state dict, rounded state dict, batch, input ids) of a Route M oracle case, made once"""
    from oracle import cases

    key = ("case", name)
    if key not in _model_cache:
        case = cases.CASES[name]
        cfg = case.make_cfg()
        sd = cases.maskgit_state_dict(cfg, case.weight_seed)
        ids_in = torch.randint(0, cfg.vocab_size + 1, (case.batch * cfg.num_cams, cfg.num_cam_tokens), generator=torch.Generator().manual_seed(5))
        _model_cache[key] = (cfg, sd, round_gemm_weights_route_m(sd), cases.inputs(case, cfg), ids_in)
    return _model_cache[key]


def oracle_forward(name, monkeypatch, products=None):
    """(logits, embed) of oracle.restate.muse_forward on the rounded-weights state dict: products=None as the oracle stands (the two-product mode's model, `lr`), else
    with restate.F replaced by single_product_functional(products) (`le`).  Evaluated once per (case, form) and left unchanged."""
    from oracle import restate as R

    key = ("forward", name, products)
    if key not in _model_cache:
        cfg, _, sdr, bt, ids_in = model_case(name)
        with monkeypatch.context() as m:
            if products is not None:
                m.setattr(R, "F", single_product_functional(products))
            _model_cache[key] = R.muse_forward(sdr, cfg, ids_in, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], depth=cfg.num_layers, heads=cfg.num_heads)
    return _model_cache[key]
