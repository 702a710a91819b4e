"""tests/golden/vq_tiny_geo.npz: the imported reference's VQModel(geometric_embedding=True) on the CPU (build container only: needs the reference tree).

Weights: cases.vq_state_dict of cases.VQ_TINY plus img_embed / cam_embed ~ N(0, 0.5^2).  Geometry per image: I_inv = diag(1/f, 1/f, 1) with f in [20, 60) and the
offsets -0.8, -0.5 in the last column; E_inv = a QR rotation and an N(0, 1) translation.  Cases (tests/test_vq_stage1_cpu.py): sq = golden vq_tiny enc_img_x with
cam_res (64, 64); rect = golden vq_rect tiny_enc_x with cam_res (24, 40); many = 49 geometries (inputs only: the tests compare the library with the restatement there).
Stored per case: the inputs and the reference's ids, emb_loss, quant and xrec = forward(x, batch)[0]; and the reference's state_dict keys and shapes, in its order.

    python tools/make_vq_geo_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import cases  # noqa: E402
from oracle.ref_import import stubs  # noqa: E402

SEED = 20240


def geometry(n, g):
    f = 20.0 + 40.0 * torch.rand(n, generator=g)
    I_inv = torch.zeros(n, 3, 3)
    I_inv[:, 0, 0] = 1 / f
    I_inv[:, 1, 1] = 1 / f
    I_inv[:, 2, 2] = 1
    I_inv[:, 0, 2] = -0.8
    I_inv[:, 1, 2] = -0.5
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=g))
    E_inv = torch.eye(4).repeat(n, 1, 1)
    E_inv[:, :3, :3] = q
    E_inv[:, :3, 3] = torch.randn(n, 3, generator=g)
    return I_inv, E_inv


def main():
    ns = stubs.import_reference()
    from multi_view_generation.modules.losses.vqperceptual import DummyLoss

    v = cases.VQ_TINY
    dd, D = v["dd"], v["dd"]["z_channels"]
    g = torch.Generator().manual_seed(SEED)
    Wimg, Wcam = 0.5 * torch.randn(D, 4, generator=g), 0.5 * torch.randn(D, 4, generator=g)
    sd = dict(cases.vq_state_dict(dd, v["n_embed"], v["embed_dim"], v["seed"], with_encoder=True))
    sd["img_embed.weight"], sd["cam_embed.weight"] = Wimg.reshape(D, 4, 1, 1), Wcam.reshape(D, 4, 1, 1)
    gold = os.path.join(ROOT, "tests", "golden")
    xs = {"sq": (np.load(os.path.join(gold, "vq_tiny.npz"))["enc_img_x"], (64, 64)), "rect": (np.load(os.path.join(gold, "vq_rect.npz"))["tiny_enc_x"], (24, 40))}
    out = {"Wimg": Wimg.numpy(), "Wcam": Wcam.numpy()}
    for name, (x, cam_res) in xs.items():
        x = torch.from_numpy(x)
        lat = (x.shape[2] // 8, x.shape[3] // 8)
        model = ns.vqgan.VQModel(ddconfig=dict(dd), lossconfig=DummyLoss(), n_embed=v["n_embed"], embed_dim=v["embed_dim"], cam_res=cam_res, cam_latent_res=lat,
                                 cam_emd_dim=D, geometric_embedding=True)
        model.load_state_dict(sd, strict=True)
        model.eval()
        I_inv, E_inv = geometry(x.shape[0], g)
        batch = {"intrinsics_inv": I_inv[None], "extrinsics_inv": E_inv[None]}      # [B = 1, cam = n, ., .]
        with torch.no_grad():
            quant, emb_loss, info = model.encode(x, batch)
            xrec, diff = model(x, batch)
        assert torch.equal(diff, emb_loss)
        out.update({name + "_I_inv": I_inv.numpy(), name + "_E_inv": E_inv.numpy(), name + "_cam_res": np.array(cam_res, dtype=np.int64),
                    name + "_ids": info[2].view(x.shape[0], -1).numpy().astype(np.int16), name + "_emb_loss": np.array(emb_loss.item(), dtype=np.float32),
                    name + "_quant": quant.numpy(), name + "_xrec": xrec.numpy()})
        if name == "sq":
            keys = list(model.state_dict())
            out["state_keys"] = np.array(keys)
            out["state_shapes"] = np.array([list(t.shape) + [0] * (4 - t.dim()) for t in model.state_dict().values()], dtype=np.int64)
            assert "image_plane" not in keys
    I_inv, E_inv = geometry(49, g)
    out.update({"many_I_inv": I_inv.numpy(), "many_E_inv": E_inv.numpy()})
    path = os.path.join(gold, "vq_tiny_geo.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
