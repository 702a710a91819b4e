"""tests/golden/vq_tiny_seg.npz: the imported reference's VQSegmentationModel(lossconfig=BCELossWithQuant()) on the CPU (build container only: needs the reference tree).

Weights: cases.vq_state_dict of cases.VQ_TINY_SEG (7 -> 7 channels, seed 77) plus colorize = randn(3, 7, 1, 1) from the generator below.  Inputs: binary 7-class layouts,
avg_pool2d(randn, 9, 1, 4) > 0.05 (blobs, occupancy about 0.30), stored as uint8.  Cases (tests/test_vq_seg_cpu.py): sq = 2 x 64 x 64, rect = 1 x 24 x 40.
Stored per case: the input and the reference's xrec and emb_loss (forward), the three values of BCELossWithQuant()(emb_loss, x, xrec, split='val'), log_images' inputs /
reconstructions and validation_step(batch, 1)['loss']; and the reference's state_dict keys and shapes, in its order.

    python tools/make_vq_seg_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import cases  # noqa: E402
from oracle.ref_import import stubs  # noqa: E402

# The comparisons of tests/test_vq_seg_cpu.py rest on a condition of the INPUT under the fp64 restatement (no library code involved): at most 1 % of the locations have one of
# their 7 logits within 1e-3 of zero.  With these weights a layout of this kind typically leaves 1.0 - 1.3 % of its locations there (seven logits meet at a location,
# 0.15 % of the logits each), so the seed is chosen by a rule: the first one from 20250 upward at which BOTH cases meet the condition.  Scanned 20250 .. 20316: 20316 is the
# only one (0.96 % and 0.94 %); e.g. 20250 gives 1.04 % and 1.04 %.
SEED = 20316
SHAPES = {"sq": (2, 64, 64), "rect": (1, 24, 40)}


def layout(n, C, H, W, g):
    return (F.avg_pool2d(torch.randn(n, C, H, W, generator=g), 9, 1, 4) > 0.05).float()


def main():
    ns = stubs.import_reference()
    from multi_view_generation.modules.losses.segmentation import BCELossWithQuant

    v = cases.VQ_TINY_SEG
    dd, C = v["dd"], v["dd"]["in_channels"]
    g = torch.Generator().manual_seed(SEED)
    colorize = torch.randn(3, C, 1, 1, generator=g)
    sd = dict(cases.vq_state_dict(dd, v["n_embed"], v["embed_dim"], v["seed"], with_encoder=True))
    sd["colorize"] = colorize
    out = {"colorize": colorize.numpy()}
    for name, (n, H, W) in SHAPES.items():
        x = layout(n, C, H, W, g)
        model = ns.vqgan.VQSegmentationModel(n_labels=C, ddconfig=dict(dd), lossconfig=BCELossWithQuant(), n_embed=v["n_embed"], embed_dim=v["embed_dim"], cam_res=(H, W),
                                             cam_latent_res=(H // 8, W // 8), cam_emd_dim=dd["z_channels"], image_key="segmentation")
        model.load_state_dict(sd, strict=True)
        model.eval()
        batch = {"segmentation": x.permute(0, 2, 3, 1).contiguous()}          # channel-last, as get_input takes it
        with torch.no_grad():
            xrec, emb_loss = model(model.get_input(batch, "segmentation"), batch)
            total, logs = model.loss(emb_loss, x, xrec, split="val")
            images = model.log_images(batch)
            val = model.validation_step(batch, 1)
        assert set(val) == {"loss"} and torch.equal(val["loss"], total)
        assert torch.equal(logs["val/total_loss"], total) and torch.equal(logs["val/quant_loss"], emb_loss)
        print(name, "occupancy %.3f" % x.mean().item(), "bce %.6f quant %.6f total %.6f" % (logs["val/bce_loss"].item(), emb_loss.item(), total.item()))
        out.update({name + "_x": x.numpy().astype(np.uint8), name + "_xrec": xrec.numpy(), name + "_emb_loss": np.array(emb_loss.item(), dtype=np.float32),
                    name + "_bce": np.array(logs["val/bce_loss"].item(), dtype=np.float32), name + "_total": np.array(total.item(), dtype=np.float32),
                    name + "_val_loss": np.array(val["loss"].item(), dtype=np.float32),
                    name + "_rgb_inputs": images["inputs"].numpy(), name + "_rgb_reconstructions": images["reconstructions"].numpy()})
        if name == "sq":
            keys = list(model.state_dict())
            out["state_keys"] = np.array(keys)
            out["state_shapes"] = np.array([list(t.shape) + [0] * (4 - t.dim()) for t in model.state_dict().values()], dtype=np.int64)
    path = os.path.join(ROOT, "tests", "golden", "vq_tiny_seg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
