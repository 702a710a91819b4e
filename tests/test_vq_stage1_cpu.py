"""Stage-1 VQGAN with the geometric embedding (VQModel(geometric_embedding=True), stage1/vqgan.py:59-69, 87-112), the codebook loss (stage1/quantize.py:290-295) and the
reconstruction forward: the cases, the fp64 restatement and the conditions that tests/test_vq_stage1_ops_gpu.py and tests/test_vq_stage1_gpu.py rest on, checked here
without a GPU.

The restatement is oracle.restate.vq_encoder + the formulas below + oracle.restate.vq_decode_ids.  It is pinned ONCE to the imported reference: tools/make_vq_geo_golden.py
runs the reference's own VQModel(geometric_embedding=True) (cases.vq_state_dict weights of cases.VQ_TINY plus the two embeddings) on the CPU and stores its ids, emb_loss,
quant and reconstruction in tests/golden/vq_tiny_geo.npz together with the inputs (Wimg, Wcam, per-image I_inv / E_inv, cam_res) and the reference's state_dict order.

The cases (one checkpoint, three inputs):
    sq     golden("vq_tiny")["enc_img_x"], 3 x 64 x 64 -> 8 x 8, cam_res (64, 64)                    192 rows
    rect   golden("vq_rect")["tiny_enc_x"], 2 x 24 x 40 -> 3 x 5, cam_res (24, 40)                    30 rows
    many   image 0 of sq x 49 (two passes of the library) with 49 different geometries               3136 rows

Conditions asserted here (test_conditions prints the figures): rows whose relative margin (d2 - d1) / max |d| is below MARGIN = 1e-4 are at most MAX_EXCLUDED = 5 %
(both numbers: tests/test_vq_encode_range_cpu.py); the embedding changes at least 10 % of the ids of every case, and building the plane with the two sides of cam_res
swapped changes at least one id of the rectangular case - so no test can pass without the embedding or with the planes mixed up.
Measured here: excluded rows sq 1.04 %, rect 0 %, many 0.57 %; ids changed by the embedding sq 39 / 192, rect 9 / 30, many 670 / 3136; swapped cam_res 1 / 30;
image 48 of `many` differs from image 0 in 17 of 64 ids; fp32 ids equal the fp64 ids on every compared row of sq and rect.

Bounds against the fixture: ids equal; xrec within 1e-5 (whole tensor, relative to max |xrec|: the decoder bound of tests/test_oracle_golden.py); emb_loss within
LOSS_RTOL = 1e-6 relative: the reference evaluates the encoder in fp32, some forty convolutions and normalisations deep, and emb_loss = 1.25 mean((z_q - z)^2) moves by
2 |dz| / |z_q - z| per element, with |z_q - z| of the order of |z| here and the signs of dz independent over the 12288 (1920) elements of the mean: forty roundings of
2^-24 adding in quadrature give 4e-7 per element and far less for the mean; 1e-6 is 17 fp32 roundings and still separates a wrong beta or divisor in the sixth digit
(measured: sq 2.7e-8, rect 9.9e-8; xrec 1.5e-6 and 1.4e-6).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle import cases
from oracle import restate as R
from test_vq_encode_range_cpu import MARGIN, MAX_EXCLUDED, relative_margins

BETA = 0.25
LOSS_RTOL = 1e-6
XREC_TOL = 1e-5
MIN_CHANGED = 0.10
CASES = ("sq", "rect", "many")
N_MANY = 49

_CACHE = {}


# ------------------------------------------------------------------------------------------------ inputs (the GPU files import everything below)
def geo_golden():
    if "g" not in _CACHE:
        _CACHE["g"] = {k: v for k, v in golden("vq_tiny_geo").items()}
    return _CACHE["g"]


def geo_sd():
    """cases.VQ_TINY's state dict plus img_embed / cam_embed of the fixture; built once and left unchanged."""
    if "sd" not in _CACHE:
        v, g = cases.VQ_TINY, geo_golden()
        sd = dict(cases.vq_state_dict(v["dd"], v["n_embed"], v["embed_dim"], v["seed"], with_encoder=True))
        D = v["dd"]["z_channels"]
        sd["img_embed.weight"] = torch.from_numpy(g["Wimg"]).reshape(D, 4, 1, 1)
        sd["cam_embed.weight"] = torch.from_numpy(g["Wcam"]).reshape(D, 4, 1, 1)
        _CACHE["sd"] = sd
    return _CACHE["sd"]


def plain_sd():
    return {k: v for k, v in geo_sd().items() if k not in ("img_embed.weight", "cam_embed.weight")}


def case_inputs(name):
    """dict(x [n, 3, H, W], I_inv [n, 3, 3], E_inv [n, 4, 4], cam_res (image_height, image_width), lat (h, w))"""
    g = geo_golden()
    if name == "sq":
        x = torch.from_numpy(golden("vq_tiny")["enc_img_x"])
    elif name == "rect":
        x = torch.from_numpy(golden("vq_rect")["tiny_enc_x"])
    else:
        x = torch.from_numpy(golden("vq_tiny")["enc_img_x"][:1]).expand(N_MANY, -1, -1, -1).contiguous()
    cam_res = tuple(int(v) for v in g[("sq" if name == "many" else name) + "_cam_res"])
    return dict(x=x, I_inv=torch.from_numpy(g[name + "_I_inv"]), E_inv=torch.from_numpy(g[name + "_E_inv"]), cam_res=cam_res, lat=(x.shape[2] // 8, x.shape[3] // 8))


def plane_of(lat, cam_res):
    """The image plane as VQModel builds it (vqgan:20-28, 59-66): [3, h w] fp32 with x = linspace(0, 1, w) image_width, y = linspace(0, 1, h) image_height,
    where image_height, image_width = cam_res."""
    h, w = lat
    image_height, image_width = cam_res
    xs, ys = torch.linspace(0, 1, w), torch.linspace(0, 1, h)
    gx, gy = torch.meshgrid(xs, ys, indexing="xy")
    return torch.stack([gx * image_width, gy * image_height, torch.ones(h, w)], 0).reshape(3, h * w)


# ------------------------------------------------------------------------------------------------ the restatement
def geo_embedding(I_inv, E_inv, plane, Wimg, Wcam, dtype=torch.float64):
    """[n, T, D]: normalize(Wimg d - Wcam c4) with d = E_inv [I_inv plane; 1], c4 = E_inv[:, :, 3], norm + 1e-7 (vqgan:96-109); plane [3, T], Wimg / Wcam [D, 4]."""
    I_inv, E_inv, plane, Wimg, Wcam = (t.to(dtype) for t in (I_inv, E_inv, plane, Wimg, Wcam))
    n, T = I_inv.shape[0], plane.shape[1]
    cam = torch.cat([I_inv @ plane, torch.ones(n, 1, T, dtype=dtype)], 1)        # [n, 4, T]
    d = E_inv @ cam                                                              # [n, 4, T]
    e = torch.einsum("od,ndt->nto", Wimg, d) - (E_inv[:, :, 3] @ Wcam.t())[:, None, :]
    return e / (e.norm(dim=-1, keepdim=True) + 1e-7)


def quant_error(z, codebook, ids, beta=BETA):
    """(row_err [rows] = sum_c (codebook[ids] - z)^2, loss = (1 + beta) mean over rows and channels) in z's dtype"""
    row = ((codebook[ids] - z) ** 2).sum(1)
    return row, (1 + beta) * row.sum() / (z.shape[0] * z.shape[1])


def quantize(sd, h, dtype):
    """quant_conv + VectorQuantizer2.forward on the encoder output h [n, C, lh, lw]: dict(ids [n, T], d [rows, n_e] direct squared distances, row_err, loss, z)"""
    z = F.conv2d(h, sd["quant_conv.weight"].to(dtype), sd["quant_conv.bias"].to(dtype))
    zf = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])
    E = sd["quantize.embedding.weight"].to(dtype)
    d = torch.sum(zf ** 2, dim=1, keepdim=True) + torch.sum(E ** 2, dim=1) - 2 * zf @ E.t()
    ids = torch.argmin(d, dim=1)
    row, loss = quant_error(zf, E, ids)
    direct = ((E[None, :, :] - zf[:, None, :]) ** 2).sum(-1)
    return dict(ids=ids.view(h.shape[0], -1), d=direct, row_err=row.view(h.shape[0], -1), loss=loss, z=zf)


def encoder_out(name, dtype=torch.float64):
    """Encoder.forward of a case's images [n, z_channels, lh, lw], computed once per (case, dtype); `many` is one image, expanded."""
    key = ("enc", "sq1" if name == "many" else name, dtype)
    if key not in _CACHE:
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in geo_sd().items()}
        x = case_inputs("sq")["x"][:1] if name == "many" else case_inputs(name)["x"]
        with torch.no_grad():
            _CACHE[key] = R.vq_encoder(sd, cases.VQ_TINY["dd"], x.to(dtype))
    h = _CACHE[key]
    return h.expand(N_MANY, -1, -1, -1) if name == "many" else h


def encode_ref(name, dtype=torch.float64, embed=True, cam_res=None):
    """VQModel.encode of a case in `dtype`: quantize()'s dict plus h_absmax (the operand of quant_conv, after the embedding) and keep [n, T] (rows whose id is compared);
    embed=False: without the embedding; cam_res: another plane."""
    key = ("ref", name, dtype, embed, cam_res)
    if key not in _CACHE:
        c = case_inputs(name)
        _CACHE[key] = encode_from(encoder_out(name, dtype), c["I_inv"], c["E_inv"], c["lat"], cam_res or c["cam_res"], dtype, embed)
    return _CACHE[key]


def encode_from(h, I_inv, E_inv, lat, cam_res, dtype=torch.float64, embed=True):
    """encode_ref's dict from an encoder output h [n, z_channels, lh, lw] and the geometry of its n images"""
    sd = geo_sd()
    if embed:
        D = h.shape[1]
        e = geo_embedding(I_inv, E_inv, plane_of(lat, cam_res), sd["img_embed.weight"].reshape(D, 4), sd["cam_embed.weight"].reshape(D, 4), dtype)
        h = h + e.reshape(h.shape[0], lat[0], lat[1], D).permute(0, 3, 1, 2)
    with torch.no_grad():
        out = quantize(sd, h, dtype)
    out["h_absmax"] = float(h.abs().max())
    out["margins"] = relative_margins(out["d"])
    out["keep"] = (out["margins"] >= MARGIN).view(out["ids"].shape)
    return out


def encode_images(x, I_inv, E_inv, cam_res, dtype=torch.float64, embed=True):
    """VQModel.encode of any images [n, 3, H, W] with one geometry per image (fp64 restatement)"""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in geo_sd().items()}
    with torch.no_grad():
        h = R.vq_encoder(sd, cases.VQ_TINY["dd"], x.to(dtype))
    return encode_from(h, I_inv.reshape(-1, 3, 3), E_inv.reshape(-1, 4, 4), (x.shape[2] // 8, x.shape[3] // 8), cam_res, dtype, embed)


def decode_ref(ids, lat, denorm=False):
    """fp32 restatement of decode_ids on given ids [n, T] (one decoder run per distinct ids: the modes mostly agree on them)"""
    key = ("dec", ids.numpy().tobytes(), tuple(lat))
    if key not in _CACHE:
        with torch.no_grad():
            _CACHE[key] = R.vq_decode_ids(geo_sd(), cases.VQ_TINY["dd"], ids, lat, denorm=False)
    return R.denormalize(_CACHE[key]) if denorm else _CACHE[key]


# conv_out x 2^14 (a power of two: the encoder output is the unscaled one times 2^14, exactly): quant_conv's operand leaves the f16 range and its site takes an exponent > 0
CONV_OUT_SCALE = 2.0 ** 14


def scaled_sd():
    if "sd_scaled" not in _CACHE:
        sd = dict(geo_sd())
        for k in ("encoder.conv_out.weight", "encoder.conv_out.bias"):
            sd[k] = sd[k] * CONV_OUT_SCALE
        _CACHE["sd_scaled"] = sd
    return _CACHE["sd_scaled"]


def scaled_quant_conv_absmax(name="sq"):
    """fp64 absmax of quant_conv's operand 2^14 h + embedding under scaled_sd()"""
    c = case_inputs(name)
    return encode_from(encoder_out(name) * CONV_OUT_SCALE, c["I_inv"], c["E_inv"], c["lat"], c["cam_res"])["h_absmax"]


def fixed_order_sum(x):
    """sum of a float32 array as the library's loss kernel forms it: element i goes to partial i % 256 in index order (double), then a binary tree over the 256 partials"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    pad = np.zeros((-len(x)) % 256)
    rows = np.concatenate([x, pad]).reshape(-1, 256)
    sh = np.zeros(256)
    for r in rows:
        sh = sh + r
    o = 128
    while o > 0:
        sh[:o] = sh[:o] + sh[o:2 * o]
        o >>= 1
    return sh[0]


def fixed_order_loss(row_err, D, beta=BETA):
    """float32 (1 + beta) / (rows D) * fixed_order_sum(row_err), bit for bit what launch_vq_loss writes"""
    row_err = np.asarray(row_err, dtype=np.float32).reshape(-1)
    scale = (1.0 + float(np.float32(beta))) / (float(len(row_err)) * float(D))
    return np.float32(fixed_order_sum(row_err) * scale)


# ------------------------------------------------------------------------------------------------ operator cases (tests/test_vq_stage1_ops_gpu.py)
GEO_SHAPES = ((2, 20, 64), (3, 7, 256), (1, 1, 32), (2, 15, 512))          # (n, T, D): 21 pixels = five full blocks and a tail block of one; D = 32: half a wave idle
QERR_SHAPES = ((5, 16, 32), (128, 64, 64), (50, 1024, 256))                 # (rows, n_e, D)
GPU_FACTOR = 4.0                                                            # GPU bound = 4 x the fp32 torch evaluation's own error (tests/test_frontend_ref_cpu.py)


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(key)) % (2 ** 31))


def geo_case(n, T, D, zero_w=False):
    g = _gen(41, n, T, D)
    f = 20.0 + 40.0 * torch.rand(n, generator=g)
    I_inv = torch.zeros(n, 3, 3)
    I_inv[:, 0, 0], I_inv[:, 1, 1], I_inv[:, 2, 2], I_inv[:, 0, 2], I_inv[:, 1, 2] = 1 / f, 1 / f, 1.0, -0.8, -0.5
    E_inv = torch.eye(4).repeat(n, 1, 1)
    E_inv[:, :3, :3] = torch.linalg.qr(torch.randn(n, 3, 3, generator=g))[0]
    E_inv[:, :3, 3] = torch.randn(n, 3, generator=g)
    plane = torch.stack([40.0 * torch.rand(T, generator=g), 24.0 * torch.rand(T, generator=g), torch.ones(T)], 0)
    w = 0.0 if zero_w else 0.5
    return dict(h=torch.randn(n, T, D, generator=g), I_inv=I_inv, E_inv=E_inv, plane=plane, Wimg=w * torch.randn(D, 4, generator=g), Wcam=w * torch.randn(D, 4, generator=g))


def geo_ref(p, dtype):
    return p["h"].to(dtype) + geo_embedding(p["I_inv"], p["E_inv"], p["plane"], p["Wimg"], p["Wcam"], dtype)


def qerr_case(rows, n_e, D, integer):
    g = _gen(43, rows, n_e, D, integer)
    if integer:
        z, cb = torch.randint(-4, 5, (rows, D), generator=g).float(), torch.randint(-4, 5, (n_e, D), generator=g).float()
    else:
        z, cb = torch.randn(rows, D, generator=g), torch.randn(n_e, D, generator=g)
    return dict(z=z, codebook=cb, ids=torch.randint(0, n_e, (rows,), generator=g))


def qerr_ref(p, dtype):
    return quant_error(p["z"].to(dtype), p["codebook"].to(dtype), p["ids"])


def rel_rows(out, ref):
    """max over rows of |out - ref| / |ref| for per-row scalars"""
    return ((out.double() - ref.double()).abs() / ref.double().abs()).max().item()


def e_cpu():
    """the fp32 torch evaluation's own error against fp64: geo (per row of D, max |.| / max |ref|) and qerr (per row, relative), the worst over the case tables"""
    from test_frontend_ref_cpu import row_err as row_rel

    e = {"geo": 0.0, "qerr": 0.0}
    for s in GEO_SHAPES:
        p = geo_case(*s)
        e["geo"] = max(e["geo"], row_rel(geo_ref(p, torch.float32), geo_ref(p, torch.float64)))
    for s in QERR_SHAPES:
        p = qerr_case(*s, integer=False)
        e["qerr"] = max(e["qerr"], rel_rows(qerr_ref(p, torch.float32)[0], qerr_ref(p, torch.float64)[0]))
    return e


def test_operator_cases():
    e = e_cpu()
    print("e_cpu", {k: f"{v:.3e}" for k, v in e.items()}, "-> GPU bounds", {k: f"{GPU_FACTOR * v:.3e}" for k, v in e.items()})
    assert all(0 < v < 1e-6 for v in e.values()), e
    for s in GEO_SHAPES:
        p = geo_case(*s)
        ref = geo_ref(p, torch.float64)
        assert ((ref - p["h"].double()).norm(dim=-1) - 1).abs().max() < 1e-6            # what is added is a unit vector
        assert torch.equal(geo_ref(geo_case(*s, zero_w=True), torch.float32), p["h"])  # 0 / (0 + 1e-7)
    for s in QERR_SHAPES:
        p = qerr_case(*s, integer=True)
        r32, l32 = qerr_ref(p, torch.float32)
        r64, l64 = qerr_ref(p, torch.float64)
        assert torch.equal(r32.double(), r64) and r64.max() <= 64 * s[2] < 2 ** 24    # integers: exact in fp32
        assert fixed_order_loss(r32.numpy(), s[2]) == np.float32(float(l64))


# ================================================================================================ the restatement against the imported reference's fixture
@pytest.mark.parametrize("name", ["sq", "rect"])
def test_restatement_matches_the_reference_fixture(name):
    g, c = geo_golden(), case_inputs(name)
    ref = encode_ref(name)
    want_ids = torch.from_numpy(g[name + "_ids"].astype(np.int64))
    assert torch.equal(ref["ids"], want_ids), f"{(ref['ids'] != want_ids).sum().item()} ids differ from the reference's"
    want_loss = float(g[name + "_emb_loss"])
    e_loss = abs(float(ref["loss"]) - want_loss) / want_loss
    # quant: the reference returns z + (z_q - z): within an ulp of z of the codebook rows
    E = geo_sd()["quantize.embedding.weight"]
    quant = E[want_ids.reshape(-1)].reshape(c["x"].shape[0], c["lat"][0], c["lat"][1], -1).permute(0, 3, 1, 2)
    e_quant = (quant - torch.from_numpy(g[name + "_quant"])).abs().max().item()
    want_x = torch.from_numpy(g[name + "_xrec"])
    e_x = ((decode_ref(want_ids, c["lat"]) - want_x).abs().max() / want_x.abs().max()).item()
    print(f"{name}: emb_loss {float(ref['loss']):.8g} vs {want_loss:.8g} (rel {e_loss:.2e}, bound {LOSS_RTOL:g}); quant {e_quant:.2e}; xrec {e_x:.2e} (bound {XREC_TOL:g})")
    assert e_loss < LOSS_RTOL
    assert e_quant <= 2.0 ** -22 * max(1.0, ref["z"].abs().max().item())
    assert e_x < XREC_TOL


@pytest.mark.parametrize("name", CASES)
def test_conditions(name):
    ref, plain = encode_ref(name), encode_ref(name, embed=False)
    rows = ref["ids"].numel()
    excluded = 1 - ref["keep"].double().mean().item()
    changed = (ref["ids"] != plain["ids"]).sum().item()
    print(f"{name}: {rows} rows, relative margin < {MARGIN:g} on {100 * excluded:.2f} %, min margin {ref['margins'].min().item():.3e}; the embedding changes {changed} ids")
    assert excluded <= MAX_EXCLUDED
    assert changed >= MIN_CHANGED * rows
    assert torch.isfinite(ref["d"]).all() and ref["h_absmax"] < 32768.0          # (f16x3r: quant_conv's exponent is 0 in every case)
    if name == "rect":
        c = case_inputs(name)
        swapped = encode_ref(name, cam_res=(c["cam_res"][1], c["cam_res"][0]))
        n_sw = (swapped["ids"] != ref["ids"]).sum().item()
        print(f"{name}: the plane of cam_res swapped changes {n_sw} ids")
        assert n_sw >= 1
    if name == "many":
        ids = ref["ids"]
        print(f"{name}: image 48 differs from image 0 in {(ids[48] != ids[0]).sum().item()} of {ids.shape[1]} ids")
        assert (ids[48] != ids[0]).any()
    else:
        ids32 = encode_ref(name, torch.float32)["ids"]
        assert torch.equal(ids32[ref["keep"]], ref["ids"][ref["keep"]])


def test_scaled_conv_out_takes_an_exponent_above_zero():
    """The checkpoint of the f16x3r test with a non-zero quant_conv exponent, and no power-of-two boundary within 1 % of the operand's absmax.  (The embedding is a unit
    vector: at this magnitude the absmax of the sum and of the encoder output alone differ by 0.03, less than the fp32 encoder's own error, so no checkpoint can make the
    exponent tell the two apart; that the exponent is taken after the add is the order of the two launches in Pass::to_latents.)"""
    from test_vq_encode_range_cpu import BOUNDARY_CLEARANCE, want_exponent

    a = scaled_quant_conv_absmax()
    print(f"quant_conv operand absmax {a:.6g} -> exponent {want_exponent(a)}")
    assert want_exponent(a) >= 1
    for j in range(0, 6):
        edge = 32768.0 * 2.0 ** j
        assert abs(a - edge) > BOUNDARY_CLEARANCE * edge
    assert torch.equal(scaled_sd()["encoder.conv_out.weight"], geo_sd()["encoder.conv_out.weight"] * CONV_OUT_SCALE)


def test_fixed_order_sum_is_a_sum():
    x = np.random.default_rng(5).random(3136).astype(np.float32)
    assert abs(fixed_order_sum(x) - float(np.sum(x.astype(np.float64)))) < 1e-9
    assert fixed_order_loss(np.full(512, 2.0, np.float32), 64) == np.float32(1.25 * 2.0 / 64)


# ================================================================================================ the drop-in module without a GPU
def _model(**kw):
    from bevgen_amd.modules.stage1.vqgan import VQModel

    v = cases.VQ_TINY
    args = dict(ddconfig=v["dd"], n_embed=v["n_embed"], embed_dim=v["embed_dim"], cam_res=(24, 40), cam_latent_res=(3, 5), cam_emd_dim=v["dd"]["z_channels"],
                geometric_embedding=True)
    args.update(kw)
    return VQModel(**args)


def test_state_dict_has_the_reference_keys_in_the_reference_order():
    g = geo_golden()
    sd = _model().state_dict()
    assert list(sd) == [str(k) for k in g["state_keys"]]
    assert [list(t.shape) + [0] * (4 - t.dim()) for t in sd.values()] == g["state_shapes"].tolist()
    assert "image_plane" not in sd
    i = list(sd).index("img_embed.weight")
    assert list(sd)[i - 1].startswith("decoder.") and list(sd)[i + 1] == "cam_embed.weight" and list(sd)[i + 2] == "quantize.embedding.weight"
    from bevgen_amd import weights as W

    v = cases.VQ_TINY
    shapes = W.vqmodel_shapes(v["dd"], v["n_embed"], v["embed_dim"], geometric=True)
    assert {k: tuple(s) for k, s in shapes.items()} == {k: tuple(t.shape) for k, t in sd.items()}
    keys = list(shapes)
    j = keys.index("img_embed.weight")
    assert keys[j - 1].startswith("decoder.") and keys[j + 1] == "cam_embed.weight" and keys[j + 2] == "quantize.embedding.weight"
    assert "img_embed.weight" not in W.vqmodel_shapes(v["dd"], v["n_embed"], v["embed_dim"])
    # the model without the embedding keeps its keys
    # the model without the embedding: the same keys without the two, in the same (the reference constructor's) order - encoder, decoder, quantize, quant_conv, post_quant_conv
    assert list(_model(geometric_embedding=False).state_dict()) == [k for k in sd if k not in ("img_embed.weight", "cam_embed.weight")]


def test_constructor_and_inputs():
    with pytest.raises(ValueError, match="cam_emd_dim"):
        _model(cam_emd_dim=32)
    m = _model()
    assert m.image_plane.shape == (1, 1, 3, 3, 5) and m.image_plane.dtype == torch.float32
    assert torch.equal(m.image_plane.reshape(3, -1), plane_of((3, 5), (24, 40)))

    class Cfg:
        cam_latent_h, cam_latent_w, cam_res = 3, 5, (24, 40)

    assert not torch.equal(m.image_plane.reshape(3, -1), R.image_plane(Cfg))       # the transformers multiply x by cam_res[0]
    x = torch.zeros(2, 3, 24, 40)
    with pytest.raises(ValueError, match="intrinsics_inv"):
        m.encode(x)
    with pytest.raises(ValueError, match="intrinsics_inv"):
        m.encode(x, {"intrinsics_inv": torch.zeros(2, 3, 3)})
    with pytest.raises(ValueError, match="matrices for 2 images"):
        m.encode(x, {"intrinsics_inv": torch.zeros(1, 3, 3, 3), "extrinsics_inv": torch.zeros(1, 3, 4, 4)})
    with pytest.raises(ValueError, match="latent grid"):
        m.encode(torch.zeros(2, 3, 64, 64), {"intrinsics_inv": torch.zeros(2, 3, 3), "extrinsics_inv": torch.zeros(2, 4, 4)})
    # [B, cam, ., .] and [(B cam), ., .] are the same rows
    from bevgen_amd.modules.stage1.vqgan import geometry_rows

    t = torch.arange(2 * 3 * 16, dtype=torch.float32).reshape(2, 3, 4, 4)
    assert torch.equal(geometry_rows(t, 4, 6), geometry_rows(t.reshape(6, 4, 4), 4, 6)) and geometry_rows(t, 4, 6).shape == (6, 4, 4)
    # get_input (vqgan:133-143)
    assert m.get_input({"image": torch.zeros(2, 3, 24, 40, 3, dtype=torch.float64)}, "image").shape == (6, 3, 24, 40)
    assert m.get_input({"image": torch.zeros(2, 24, 40)}, "image").shape == (2, 1, 24, 40)
    out = m.get_input({"image": torch.zeros(2, 24, 40, 3, dtype=torch.uint8)}, "image")
    assert out.shape == (2, 3, 24, 40) and out.dtype == torch.float32 and out.is_contiguous()
    with pytest.raises(NotImplementedError, match="to_rgb"):
        m.log_images({"image": torch.zeros(1, 24, 40, 7)})
    # without a device the forward is an error, not a fallback
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(x, {"intrinsics_inv": torch.zeros(2, 3, 3), "extrinsics_inv": torch.zeros(2, 4, 4)})


REF_CONFIGS = "/root/reference/configs"


@pytest.mark.reference
@pytest.mark.skipif(not os.path.isdir(REF_CONFIGS), reason="needs /root/reference (build container only)")
def test_hydra_lite_instantiates_the_stage_1_camera_config():
    from bevgen_amd import hydra_lite as H
    from bevgen_amd.modules.stage1.vqgan import VQModel

    node = H._load_file(H.Path(REF_CONFIGS) / "model" / "stage_1_cam.yaml")[2]
    assert node["geometric_embedding"] is True and node["cam_emd_dim"] == node["ddconfig"]["z_channels"] == 256
    # the file at a fraction of its width (the constructor is what is under test, not 70 M parameters); cam_res / cam_latent_res as configs/train.yaml interpolates them
    node = dict(node, cam_res=[256, 256], cam_latent_res=[16, 16], cam_emd_dim=32, embed_dim=32, n_embed=16, ddconfig=dict(node["ddconfig"], ch=32, z_channels=32))
    m = H.instantiate(node)
    assert type(m) is VQModel and m.geometric_embedding and m.image_plane.shape == (1, 1, 3, 16, 16)
    assert m.state_dict()["img_embed.weight"].shape == (32, 4, 1, 1)


# ================================================================================================ plumbing
def test_header_and_binding_carry_the_new_entries():
    from bevgen_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    for name, nargs in (("bevgen_vq_encode_ex", 13), ("bevgen_op_vq_geo_embed", 11), ("bevgen_op_vq_quant_error", 11)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m and len(m.group(1).split(",")) == nargs, name
    m = re.search(r"#define\s+BEVGEN_ABI_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.ABI_VERSION == 10
    assert ctypes.sizeof(_lib.bevgen_cfg) == 4 * (3 + 5 + 3 + 3 + 3 + 2 + 8 + 8 + 1 + 16)
    assert len(_lib.SIGNATURES["bevgen_vq_encode"][1]) == 7
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib = _lib.load()
    for name in ("bevgen_vq_encode_ex", "bevgen_op_vq_geo_embed", "bevgen_op_vq_quant_error"):
        assert hasattr(lib, name)
