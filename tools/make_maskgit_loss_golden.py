"""tests/golden/route_m_loss.npz: the imported reference's MaskGit.forward (muse_net:629-729, eval mode, self token critic) on the CPU (build container only: needs the
reference tree).  Nothing of the reference is edited; its four noise sources are patched for the duration of a call: muse_net.uniform (mask times), torch.rand (the
permutation's uniforms), muse_net.random (the sampling temperature) and muse_net.gumbel_noise (built from the stored uniforms); SelfCritic.forward is wrapped to record
the critic input and its labels.

Cases (tests/maskgit_loss_common.py LOSS_CASES; weights regenerated from the case's seeds as everywhere else): m_tiny_rays (B = 2, 3 cameras), m_tiny_6cam (B = 1, six
cameras), m_fold (D = 192: folded LayerNorms and GEGLU epilogue of the HIP path), m_tiny_heavy (heavy-tailed weights).  Stored per case: ids, time_u, perm_u, gumbel_u,
temperature; the reference's mask, x, critic_input and labels; its three losses and the ce of a train_only_generator=True call; max |logit| and max |critic logit| of the
fp64 restatement (the tolerances of tests/test_maskgit_loss_gpu.py are multiples of them).  Arrays only.

The comparisons rest on two conditions of the INPUTS, decided by the fp64 restatement alone (no library code): the uniforms within every perm_u row are distinct, and at
every masked position the top-2 margin of logits / temperature + gumbel is >= 1e-3.  The noise seed of a case is the first one from SEED_START = 20260 upward that meets
both (and, by construction of time_u, has rows with n = 1, n = T and counts between).  Scanned 20260 .. 20260 for every case: the first seed meets the conditions in all
four (rows of T = 16 distinct uniforms; margins m_tiny_rays 4.68e-2, m_tiny_6cam 2.56e-2, m_fold 4.50e-2, m_tiny_heavy 1.60e+2 - its logits reach 458); counts per row
16, 1, 10, 13, 2, 11 (53 of 96 positions masked).  The seeds are recorded in tests/maskgit_loss_common.py LOSS_CASES and asserted here.

    python tools/make_maskgit_loss_golden.py
"""
import os
import sys
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import maskgit_loss_common as M  # noqa: E402
from oracle.ref_import import refmodels, stubs  # noqa: E402


def pick_seed(name, limit=200):
    for seed in range(M.SEED_START, M.SEED_START + limit):
        inp = M.draw_inputs(name, seed)
        r = M.restate(name, inp)
        distinct, margin_ok = M.input_conditions(inp, r)
        print(f"{name}: seed {seed}: distinct {distinct}, margin {r['margin']:.3e}, counts {[int(v) for v in r['n']]}")
        if distinct and margin_ok and M.count_conditions(inp):
            return seed, inp, r
    raise RuntimeError(f"{name}: no seed in [{M.SEED_START}, {M.SEED_START + limit}) meets the input conditions")


def reference_losses(name, inp, train_only_generator=False):
    case, cfg, sd, bt = M.model(name)
    mg, _ = refmodels.build_ref_maskgit(cfg, sd)
    mn = stubs.import_reference().muse_net
    rec = {}
    critic_forward = type(mg.token_critic).forward

    def recording_forward(self, x, *a, **k):
        rec["critic_input"], rec["labels"] = x.clone(), k["labels"].clone()
        return critic_forward(self, x, *a, **k)

    def gumbel(t):
        return -mn.log(-mn.log(inp["gumbel_u"].reshape(t.shape)))

    net_forward = type(mg.transformer).forward

    def recording_net_forward(self, x, *a, **k):   # the first call of a MaskGit.forward receives x = where(mask, mask_id, ids): the reference's mask is x == mask_id
        rec.setdefault("x", x.clone())
        return net_forward(self, x, *a, **k)

    with mock.patch.object(mn, "uniform", lambda shape, **k: inp["time_u"].clone()), mock.patch.object(torch, "rand", lambda *a, **k: inp["perm_u"].clone()), \
         mock.patch.object(mn, "random", lambda: inp["temperature"]), mock.patch.object(mn, "gumbel_noise", gumbel), \
         mock.patch.object(type(mg.token_critic), "forward", recording_forward), mock.patch.object(type(mg.transformer), "forward", recording_net_forward), torch.no_grad():
        out = mg(inp["ids"], cond_images=bt["cond_ids"], batch={"intrinsics_inv": bt["intrinsics_inv"], "extrinsics_inv": bt["extrinsics_inv"]},
                 train_only_generator=train_only_generator)
    return out, rec


def cfg_vocab(name):
    return M.model(name)[1].vocab_size


def main():
    out, table = {}, []
    for name in M.LOSS_CASES:
        seed, inp, r = pick_seed(name)
        assert seed == M.LOSS_CASES[name], f"{name}: the rule gives seed {seed}, tests/maskgit_loss_common.py says {M.LOSS_CASES[name]}: update the table"
        (loss, ce, bce), rec = reference_losses(name, inp)
        ce_only, _ = reference_losses(name, inp, train_only_generator=True)
        assert torch.equal(ce_only, ce)
        ci, labels, x = rec["critic_input"], rec["labels"], rec["x"]
        mask = x == cfg_vocab(name)
        assert torch.equal(x, r["x"]) and torch.equal(mask, r["mask"]), f"{name}: the restatement's mask differs from the reference's"
        assert torch.equal(ci, r["critic_input"]) and torch.equal(labels.double(), r["labels"]), f"{name}: the restatement's critic input differs from the reference's"
        rel = lambda a, b: abs(a.item() - b.item()) / abs(b.item())
        assert rel(ce, r["ce"]) < M.LOSS_RTOL and rel(bce, r["bce"]) < M.LOSS_RTOL and rel(loss, r["loss"]) < M.LOSS_RTOL, (name, ce, r["ce"], bce, r["bce"])
        table.append(f"{name}: seed {seed} (scanned {M.SEED_START} .. {seed}), margin {r['margin']:.3e}, masked {int(mask.sum())}, loss {loss.item():.6f} ce {ce.item():.6f} "
                     f"bce {bce.item():.6f}, max |logit| {r['max_logit']:.2f}, max |critic logit| {r['max_critic_logit']:.3f}")
        f32 = lambda v: np.array(float(v), dtype=np.float32)
        out.update({name + "_ids": inp["ids"].numpy().astype(np.int16), name + "_time_u": inp["time_u"].numpy(), name + "_perm_u": inp["perm_u"].numpy(),
                    name + "_gumbel_u": inp["gumbel_u"].numpy(), name + "_temperature": np.array(inp["temperature"], dtype=np.float64),
                    name + "_mask": mask.numpy(), name + "_x": x.numpy().astype(np.int16), name + "_critic_input": ci.numpy().astype(np.int16),
                    name + "_labels": labels.numpy().astype(np.uint8), name + "_loss": f32(loss), name + "_ce": f32(ce), name + "_bce": f32(bce), name + "_ce_only": f32(ce_only),
                    name + "_max_logit": np.array(r["max_logit"]), name + "_max_critic_logit": np.array(r["max_critic_logit"])})
    np.savez_compressed(M.GOLDEN, **out)
    print("\n".join(table))
    print(M.GOLDEN, os.path.getsize(M.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
