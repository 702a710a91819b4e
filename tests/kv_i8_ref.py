"""The int8 KV-cache format (kv_dtype 2, include/bevgen_hip.h BEVGEN_KV_I8) restated in torch fp32 on the CPU: a helper of the test_kv_i8_* modules, not a test.

One buffer (K or V of one layer) = [B, H, Lmax, 64] int8 codes followed immediately by [B, H, Lmax] fp32 row scales: 68 B H Lmax bytes, the scale plane at byte
64 B H Lmax.  Quantiser of one 64-element row, every operation one correctly rounded IEEE fp32 operation (so the device must produce the same bytes):
    amax = max |r_i|;  amax < 1e-30: codes 0, scale 0;  else scale = amax / 127, inv = 127 / amax, code_i = clamp(rint(r_i * inv), -127, 127) (nearest even);
    value read back = code_i * scale.
"""
import torch

ROW_BYTES = 68


def quantise(values):
    """values [..., 64] fp32 -> (codes int8 [..., 64], scales fp32 [...])"""
    v = values.to(torch.float32)
    amax = v.abs().amax(-1)
    live = amax >= 1e-30
    safe = torch.where(live, amax, torch.ones_like(amax))
    scale = torch.where(live, safe / torch.tensor(127.0), torch.zeros_like(amax))
    inv = torch.tensor(127.0) / safe
    codes = torch.round(v * inv.unsqueeze(-1)).clamp(-127.0, 127.0)       # torch.round: half to even
    codes = torch.where(live.unsqueeze(-1), codes, torch.zeros_like(codes))
    return codes.to(torch.int8), scale


def pack_planes(codes, scales):
    """codes int8 [..., Lmax, 64] + scales fp32 [..., Lmax] -> the flat uint8 buffer"""
    return torch.cat([codes.contiguous().view(torch.uint8).reshape(-1), scales.contiguous().view(torch.uint8).reshape(-1)])


def pack(values):
    """values [..., Lmax, 64] (fp32; leading dimensions = B, H) -> flat uint8 buffer of 68 x rows bytes"""
    return pack_planes(*quantise(values))


def unpack(buffer, B, H, Lmax):
    """flat uint8 buffer -> (codes int8 [B, H, Lmax, 64], scales fp32 [B, H, Lmax], dequantised fp32 [B, H, Lmax, 64])"""
    rows = B * H * Lmax
    buffer = buffer.detach().cpu().contiguous().view(torch.uint8).reshape(-1)
    assert buffer.numel() == ROW_BYTES * rows, f"{buffer.numel()} bytes for {rows} rows"
    codes = buffer[:64 * rows].clone().view(torch.int8).reshape(B, H, Lmax, 64)
    scales = buffer[64 * rows:].clone().view(torch.float32).reshape(B, H, Lmax)
    return codes, scales, codes.to(torch.float32) * scales.unsqueeze(-1)


# ---- the oracle's Route A restatement with an int8 KV cache (wrapped from the test side: oracle/ stays as it is)
class _I8Rows(list):
    """ARCache.k / ARCache.v: a layer's rows pass through the quantiser when they are stored.  The prefill's own attention still reads the exact rows it has just
    computed (the device prefill reads exact fp32 K / V from a scratch pair); every later read - the decode steps, the new key included - sees code * scale."""

    def __init__(self):
        super().__init__()
        self._fresh = set()

    @staticmethod
    def _deq(t):
        codes, scales = quantise(t)
        return codes.to(torch.float32) * scales.unsqueeze(-1)

    def append(self, t):
        self._fresh.add(len(self))
        super().append(t)

    def __getitem__(self, i):
        t = super().__getitem__(i)
        if i in self._fresh:                                   # the prefill's read: exact this once, stored quantised
            self._fresh.discard(i)
            super().__setitem__(i, self._deq(t))
        return t

    def __setitem__(self, i, t):                               # ARCache._block: self.k[i] = cat([self.k[i], new row])
        old = super().__getitem__(i)
        super().__setitem__(i, torch.cat([old, self._deq(t[:, :, old.shape[2]:])], dim=2))


def i8_cache_class(base):
    """base = oracle.restate.ARCache -> the same class whose k / v lists quantise what they store"""

    class I8Cache(base):
        k = property(lambda self: self._k8, lambda self, value: setattr(self, "_k8", _I8Rows()))
        v = property(lambda self: self._v8, lambda self, value: setattr(self, "_v8", _I8Rows()))

    return I8Cache


def teacher_forced_logits(cache, cfg, teacher):
    """[N, B, V]: every step's logits with the tokens `teacher` [B, C, T] fed back (the loop of oracle.restate.ar_sample_cached)"""
    T, out = cfg.num_cam_tokens, []
    for s in range(cfg.num_img_tokens):
        out.append(cache.logits().clone())
        if s + 1 < cfg.num_img_tokens:
            j = int(cfg.forward_shuffle_idx[s])
            cache.append(s, teacher[:, j // T, j % T])
    return torch.stack(out)


def step_distance(logits, ref):
    """worst per-step relative distance of [N, B, V] logits: max over steps of max |a - b| / max |b|"""
    return max(((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item() for a, b in zip(logits, ref))
