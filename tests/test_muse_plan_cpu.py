"""How a Route M forward launches its projections (bevgen_amd/csrc/muse_plan.h) on the CPU: k slices, key ranges and the stream-K / split-K / fused decision per projection.

tests/host/muse_plan_dump.cpp is built for the host only, with the address and undefined-behaviour sanitizers, and run directly: no GPU and no HIP call.  The expected
decisions are for the bench model (D = 1024, H = 16, Fpad = 2752, six views: 1536 token rows per scene, 49 self-attention key tiles); they were derived by hand from the
driver these functions were taken out of and confirmed against a copy of its own rule code (experiments/r13.md)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

D, FPAD = 1024, 2752
OUT, Q, KV, GEGLU, UP = range(5)   # MuseProj


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("muse_plan") / "muse_plan_dump")
    r = subprocess.run([HIPCC, "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", os.path.join(ROOT, "bevgen_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined",
                        os.path.join(ROOT, "tests", "host", "muse_plan_dump.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        """one process for all `cases`; returns one result per case"""
        p = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])   # (a sanitizer report goes to stderr)
        out = [json.loads(line) for line in p.stdout.splitlines()]
        assert len(out) == len(cases) and not any("error" in o for o in out), out
        return out

    return run


def _proj(kind, M, N, K, **kw):
    return f"proj kind={kind} M={M} N={N} K={K} " + " ".join(f"{k.replace('__', '.')}={v}" for k, v in kw.items())


def _layer(rows, fold, **kw):
    """the projections of one layer at fold level `fold`, merged q|k|v, as the driver presents them (fold roles: muse.cpp)"""
    f2 = int(fold == 2)
    return {
        "qkv": _proj(KV, rows, 3 * D, D, merged=1, fold=f2, **kw),     # (consumer only behind a producing layer; the role never matters for this row)
        "out_self": _proj(OUT, rows, D, D, fold=f2, **kw),
        "q_cross": _proj(Q, rows, D, D, fold=f2, **kw),
        "out_cross": _proj(OUT, rows, D, D, fold=f2, **kw),
        "up": _proj(GEGLU, rows, 2 * FPAD, D, fold=int(fold >= 1), **kw),
        "down": _proj(OUT, rows, D, FPAD, fold=int(fold >= 1), **kw),
    }


def _run_layer(dump, rows, fold, **kw):
    cases = _layer(rows, fold, **kw)
    return dict(zip(cases, dump(list(cases.values()))))


FUSED = {"sk_asked": 0, "sk": 0, "kpart": 0, "ksplit": 1, "q_unfused": 0, "force_wm": 0}


def test_pick_ksplit(dump):
    shapes = [(1536, 1024, 1024), (1536, 1024, 2752), (2304, 1024, 2752), (2304, 1024, 1024), (3072, 1024, 2752), (24576, 1024, 1024)]
    got = dump([f"ksplit rows={r} N={n} K={k}" for (r, n, k) in shapes])
    assert [g["ksplit"] for g in got] == [1, 1, 2, 1, 1, 1]   # 96 tiles <= 128 | 144 tiles, K >= 2048 | K < 2048 | 192 tiles >= 160 | the chip is full
    pinned = dump(["ksplit rows=1536 N=1024 K=1024 sw.ksplit=2", "ksplit rows=1536 N=1024 K=96 sw.ksplit=6", "ksplit rows=1536 N=1024 K=2752 sw.ksplit=9",
                   "ksplit rows=24576 N=1024 K=1024 sw.ksplit=2"])
    assert [g["ksplit"] for g in pinned] == [2, 1, 6, 1]   # three k-tiles: no slice gets two | the workspace holds six slices | a full chip is never split


def test_pick_attn_ksplit(dump):
    got = dump(["attn blocks=96 tiles=49", "attn blocks=192 tiles=49", "attn blocks=48 tiles=25", "attn blocks=96 tiles=49 sw.attn_ksplit=8",
                "attn blocks=1536 tiles=49 sw.attn_ksplit=1", "attn blocks=96 tiles=5 sw.attn_ksplit=8"])
    assert [g["attn_ksplit"] for g in got] == [2, 1, 3, 8, 1, 5]


def test_split_k_workspace_exists_only_where_a_projection_is_split(dump):
    got = dump([f"kpart rows={r} D={D} Fpad={FPAD}" for r in (1536, 2304, 3072, 24576)] + [f"kpart rows=1536 D={D} Fpad={FPAD} sw.ksplit=2",
                                                                                         f"kpart rows=24576 D={D} Fpad={FPAD} sw.ksplit=2"])
    assert [g["kpart"] for g in got] == [0, 1, 0, 0, 1, 0]


def test_default_switches_one_scene_every_projection_is_one_fused_launch(dump):
    for fold in (0, 1, 2):
        for name, r in _run_layer(dump, 1536, fold, kpart=0, sk_ws=1).items():   # (no split-K workspace at 1536 rows; the stream-K one is carved whatever the switch says)
            assert r == dict(FUSED, force_wm=4 if name == "qkv" else 0), (fold, name, r)


def test_one_and_a_half_scenes_split_the_down_projection_only(dump):
    l0, l1 = (_run_layer(dump, 2304, fold, kpart=1, sk_ws=1) for fold in (0, 1))
    assert (l0["down"]["ksplit"], l0["down"]["kpart"]) == (2, 1)
    assert l1["down"] == FUSED                                                 # consumer of the inner LayerNorm: keeps its epilogue
    assert l0["out_self"] == l0["out_cross"] == dict(FUSED, kpart=1)           # handed the workspace, one slice
    assert l0["q_cross"] == l1["q_cross"] == FUSED
    assert l0["qkv"] == dict(FUSED, force_wm=4) and l0["up"] == l1["up"] == FUSED


def test_ksplit_switch(dump):
    l0, l2 = (_run_layer(dump, 1536, fold, kpart=1, sk_ws=1, sw__ksplit=2) for fold in (0, 2))
    for name in ("out_self", "out_cross", "down"):
        assert l0[name] == dict(FUSED, kpart=1, ksplit=2), name
    assert l0["q_cross"] == dict(FUSED, kpart=1, ksplit=2, q_unfused=1)        # un-fused projection + the query preparation kernel
    assert l2["q_cross"] == FUSED and l2["down"] == FUSED                      # fold roles keep the fused epilogue
    assert l2["out_self"] == l2["out_cross"] == FUSED                          # (producers at level 2)
    # the un-merged self-attention q behaves like the cross one; k|v and q|k|v never split
    q_self, kv = dump([_proj(Q, 1536, D, D, kpart=1, sw__ksplit=2), _proj(KV, 1536, 2 * D, D, kpart=1, sw__ksplit=2)])
    assert q_self == l0["q_cross"] and kv == FUSED and l0["qkv"] == dict(FUSED, force_wm=4) and l0["up"] == FUSED


def test_stream_k_switch(dump):
    one = _run_layer(dump, 1536, 1, kpart=0, sk_ws=1, gsw__sk=1)
    assert one["qkv"] == dict(FUSED, sk_asked=1, sk=1, force_wm=4) and one["up"] == dict(FUSED, sk_asked=1, sk=1)   # 144 tiles | 258 tiles
    for name in ("out_self", "q_cross", "out_cross", "down"):
        assert one[name] == FUSED, name                                        # 48 tiles
    for name, r in _run_layer(dump, 24576, 1, kpart=0, sk_ws=0, gsw__sk=1).items():
        assert r == dict(FUSED, force_wm=4 if name == "qkv" else 0), name      # whole rounds (or the row split): none
    # asked without a workspace: nothing is carried ...
    assert dump([_proj(KV, 1536, 3 * D, D, merged=1, sk_ws=0, gsw__sk=1)])[0] == dict(FUSED, sk_asked=1, force_wm=4)
    # ... and the ask alone keeps the split-K workspace away from the launch ([4096, 1024]: 128 tiles, half of the round empty)
    asked, free = dump([_proj(OUT, 4096, D, D, kpart=1, sk_ws=0, gsw__sk=1), _proj(OUT, 4096, D, D, kpart=1, sk_ws=0)])
    assert asked == dict(FUSED, sk_asked=1) and free == dict(FUSED, kpart=1)
    assert dump([_proj(Q, 4096, D, D, kpart=1, sk_ws=1, gsw__sk=1, sw__ksplit=2)])[0] == dict(FUSED, sk_asked=1, sk=1)
    # the up-projection without the GEGLU weight order asks for nothing, whatever the switches say
    assert dump([_proj(UP, 1536, 5460, D, kpart=1, sk_ws=1, gsw__sk=1, sw__ksplit=2)])[0] == FUSED


def test_merge_and_fold_rules(dump):
    got = dump(["rules rows=1536", "rules rows=3072", "rules rows=4608", "rules rows=24576 sw.ln_fold=2 sw.ln_merge=1 sw.qkv_merge=3", "rules rows=1536 sw.ln_merge=0 sw.qkv_merge=0",
                "rules rows=3072 sw.qkv_merge=3 sw.ln_fold=7", "rules rows=1536 sw.ln_fold=2 consts=0", "rules rows=1536 sw.ln_fold=-1"])
    assert [(g["fold"], g["tile_merge"], g["qkv_merged"]) for g in got] == [(1, 1, 1), (1, 1, 1), (1, 0, 1), (2, 1, 0), (1, 0, 0), (2, 1, 1), (0, 1, 1), (0, 1, 1)]
    # $BEVGEN_QKV_WM4 = 0: the merged projection does not pin its block shape; the un-merged k|v never does
    assert [r["force_wm"] for r in dump([_proj(KV, 1536, 3 * D, D, merged=1, sw__qkv_wm4=0), _proj(KV, 1536, 2 * D, D), _proj(KV, 1536, 3 * D, D, merged=1)])] == [0, 0, 4]
