"""The int8 decode-weight format (decode_weights='i8', include/bevgen_hip.h BEVGEN_W_I8) restated in torch fp32 on the CPU: a helper of the test_decode_w_i8_* modules,
not a test.

One projection matrix W [N, K] = int8 codes [N, K] + one fp32 scale per output row.  Quantiser of the row W[n, :], the rule of the int8 KV cache (tests/kv_i8_ref.py)
with the row of a matrix in place of a 64-element cache row; every operation one correctly rounded IEEE fp32 operation, so the device must produce the same bytes:
    amax = max_k |W[n, k]|;  amax < 1e-30: codes 0, scale 0;  else scale = amax / 127, inv = 127 / amax, code = clamp(rint(w * inv), -127, 127) (nearest even);
    value = code * scale.
"""
import torch

import kv_i8_ref as Q


def quantise_rows(w):
    """w [N, K] fp32 -> (codes fp32 [N, K] holding integers in [-127, 127], scales fp32 [N], dequantised fp32 [N, K] = code * scale)"""
    codes, scales = Q.quantise(w)                              # (the cache quantiser works on the last dimension, whatever its length)
    codes = codes.to(torch.float32)
    return codes, scales, codes * scales.unsqueeze(-1)


def is_projection_weight(key):
    """the matrices the mode quantises: q / k / v, both MLP matrices of every block, and the head"""
    return key == "head.weight" or (key.startswith("blocks.") and key.endswith(".weight") and
                                    any(t in key for t in (".attention.query.", ".attention.key.", ".attention.value.", ".mlp.0.", ".mlp.2.")))


def quantize_projection_weights_i8(sd):
    """The model decode_weights='i8' defines: every projection matrix replaced by code * scale, one scale per output row (everything else untouched).  The library
    quantises the fused q | k | v matrix [3 D, D] row by row, which is each [D, D] matrix row by row: the three are quantised separately here."""
    out = dict(sd)
    for k, v in sd.items():
        if is_projection_weight(k):
            out[k] = quantise_rows(v.to(torch.float32))[2]
    return out
