"""Launch plan of the LDS-DMA GEMM (bevgen_amd/csrc/gemm_plan.h) on the CPU: which instantiation, grid, block size and LDS size a problem gets.

tests/host/gemm_plan_dump.cpp is built for the host only, with the address and undefined-behaviour sanitizers, and run directly: no GPU and no HIP call.  The expected plans
were derived by hand from the launcher this header replaced (default switches, 256 CUs, fp32 weights, 16-byte-aligned pointers, ldr = N)."""
import itertools
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

QKV = "epi=4 epi_rows=1536 force_wm=4"
# case -> launches: (first row, end row, <MODE, WM, S, KS, TI, TJ>, grid, threads, LDS bytes, profiler kind)
EXPECTED = {
    "M=24576 N=1024 K=1024 R=1": [(0, 24576, (0, 4, 3, 0, 2, 2), (8, 96, 1), 512, 153600, "G")],
    f"M=24576 N=3072 K=1024 {QKV}": [(0, 24576, (0, 4, 3, 0, 2, 2), (24, 96, 1), 512, 147456, "G")],
    "M=24576 N=5504 K=1024 epi=2": [(0, 24320, (0, 4, 3, 0, 2, 2), (43, 95, 1), 512, 147456, "G"), (24320, 24576, (0, 1, 4, 0, 1, 2), (43, 4, 1), 256, 98304, "S")],
    f"M=3072 N=3072 K=1024 {QKV}": [(0, 2560, (0, 4, 3, 0, 2, 2), (24, 10, 1), 512, 147456, "G"), (2560, 3072, (0, 1, 4, 0, 1, 2), (24, 8, 1), 256, 98304, "S")],
    f"M=1536 N=3072 K=1024 {QKV}": [(0, 1536, (0, 4, 3, 0, 2, 2), (24, 6, 1), 512, 147456, "G")],
    "M=1536 N=5504 K=1024 epi=2": [(0, 1280, (0, 4, 3, 0, 2, 2), (43, 5, 1), 512, 147456, "G"), (1280, 1536, (0, 1, 4, 0, 1, 2), (43, 4, 1), 256, 98304, "S")],
    "M=1536 N=1024 K=1024 R=1": [(0, 1536, (0, 1, 4, 0, 1, 1), (8, 24, 1), 512, 104448, "S")],
    "M=1536 N=1024 K=1024 epi=1": [(0, 1536, (0, 1, 4, 0, 1, 2), (8, 24, 1), 256, 98304, "S")],
    "M=1536 N=1024 K=2752 R=1 ln_in_gsums=1": [(0, 1536, (0, 1, 4, 0, 1, 1), (8, 24, 1), 512, 112640, "S")],
    "M=3072 N=1024 K=2752 R=1 ksplit=2 kpart=1": [(0, 3072, (0, 2, 2, 1, 2, 2), (8, 24, 2), 256, 71680, "S")],
    "M=6144 N=1024 K=1024 R=1": [(0, 6144, (0, 2, 2, 0, 2, 2), (8, 48, 1), 256, 71680, "S")],
    "M=12288 N=1024 K=1024 R=1": [(0, 8192, (0, 4, 3, 0, 2, 2), (8, 32, 1), 512, 153600, "G"), (8192, 12288, (0, 2, 4, 0, 1, 2), (8, 32, 1), 512, 137216, "S")],
    "M=8485 N=1024 K=256 R=1": [(0, 8192, (0, 4, 3, 0, 2, 2), (8, 32, 1), 512, 153600, "G"), (8192, 8485, (0, 1, 4, 0, 1, 1), (8, 5, 1), 512, 104448, "S")],
    "M=333 N=264 K=96 R=1": [(0, 333, (0, 1, 4, 0, 1, 1), (3, 6, 1), 512, 104448, "S")],
    "M=128 N=128 K=32": [(0, 128, (0, 1, 4, 0, 1, 1), (1, 2, 1), 512, 98304, "S")],
    "conv=1 n=48 h=16 w=16 cin=512 N=512": [(0, 12288, (2, 2, 2, 0, 2, 2), (4, 96, 1), 256, 65536, "C")],
    "conv=1 n=1 h=16 w=16 cin=128 N=128": [(0, 256, (2, 2, 4, 0, 1, 2), (1, 2, 1), 512, 131072, "C")],
    "conv=1 up=1 n=6 h=32 w=32 cin=256 N=256": [(0, 6144, (1, 2, 4, 0, 1, 2), (2, 48, 1), 512, 131072, "C")],
    "conv=1 n=96 h=64 w=64 cin=128 N=128": [(0, 393216, (2, 4, 3, 0, 2, 2), (1, 1536, 1), 512, 147456, "C")],
}
RESIDUAL_CASES = [c for c in EXPECTED if "R=1" in c]
CONV_ONE_IMAGE = "conv=1 n=1 h=16 w=16 cin=128 N=128"


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_dump")
    r = subprocess.run([HIPCC, "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", os.path.join(ROOT, "bevgen_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined",
                        os.path.join(ROOT, "tests", "host", "gemm_plan_dump.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        """one process for all `cases`; returns (one result per case, the variant table)"""
        p = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])   # (a sanitizer report goes to stderr)
        out = [json.loads(line) for line in p.stdout.splitlines()]
        assert len(out) == len(cases) + 1, (len(out), len(cases))
        return out[:-1], [tuple(t) for t in out[-1]["table"]]

    return run


def _launches(res, w16=0):
    assert "launches" in res, res
    for l in res["launches"]:
        assert l["w16"] == w16 and l["sk"] == 0, l
    return [(l["rows"][0], l["rows"][1], tuple(l["variant"]), tuple(l["grid"]), l["threads"], l["lds"], l["prof"]) for l in res["launches"]]


def _key(l):   # a launch as a row of the table: (MODE, WM, S, W16, KS, TI, TJ, SK)
    m, wm, s, ks, ti, tj = l["variant"]
    return (m, wm, s, l["w16"], ks, ti, tj, l["sk"])


def test_variant_table_is_the_26_plus_2_instantiations(dump):
    _, table = dump([])
    assert len(table) == 28 and len(set(table)) == 28
    tuples = {(m, wm, s, ks, ti, tj, sk) for (m, wm, s, w16, ks, ti, tj, sk) in table}
    assert len(tuples) == 14 and all((m, wm, s, w16, ks, ti, tj, sk) in table for (m, wm, s, ks, ti, tj, sk) in tuples for w16 in (0, 1))   # every tuple x W16
    assert sorted(t for t in tuples if t[-1]) == [(0, 4, 3, 0, 2, 2, 1)]


@pytest.mark.parametrize("w16", [0, 1])
def test_expected_plans(dump, w16):
    cases = list(EXPECTED)
    res, _ = dump([f"{c} w16={w16}" for c in cases])
    for c, r in zip(cases, res):
        assert _launches(r, w16) == EXPECTED[c], c
        assert [l["reduce"] for l in r["launches"]] == [int("ksplit=2" in c)] * len(r["launches"]), c
        assert r["xcd_calls"] == 0, c


def test_switches(dump):
    cases = list(EXPECTED)

    def one(case):
        return dump([case])[0][0]

    assert _launches(one("M=24576 N=5504 K=1024 epi=2 sw.rowsplit=0")) == [(0, 24576, (0, 4, 3, 0, 2, 2), (43, 96, 1), 512, 147456, "G")]
    assert _launches(one("M=1536 N=1024 K=1024 R=1 sw.stages=2")) == [(0, 1536, (0, 2, 2, 0, 2, 2), (8, 12, 1), 256, 71680, "S")]
    ks = "M=3072 N=1024 K=2752 R=1 ksplit=2 kpart=1"
    assert _launches(one(ks + " sw.stages=16")) == EXPECTED[ks]   # 64-row blocks have no split-K form: the pin is ignored
    assert _launches(one("M=24576 N=1024 K=1024 sw.wm=2")) == [(0, 24576, (0, 2, 2, 0, 2, 2), (8, 192, 1), 256, 65536, "S")]
    # half8 = 0: every eight-wave 64-row block becomes the four-wave one, nothing else moves
    for c, r in zip(cases, dump([c + " sw.half8=0" for c in cases])[0]):
        want = [(a, b, (0, 1, 4, 0, 1, 2), g, 256, lds, p) if v == (0, 1, 4, 0, 1, 1) else (a, b, v, g, t, lds, p) for (a, b, v, g, t, lds, p) in EXPECTED[c]]
        assert _launches(r) == want, c
    # conv_fast = 0: the general convolution variant where the stride-1 one is picked
    for c, r in zip(cases, dump([c + " sw.conv_fast=0" for c in cases])[0]):
        want = [(a, b, (1,) + v[1:] if v[0] == 2 else v, g, t, lds, p) for (a, b, v, g, t, lds, p) in EXPECTED[c]]
        assert _launches(r) == want, c
    assert _launches(one(CONV_ONE_IMAGE + " sw.conv_thin=0")) == [(0, 256, (2, 2, 2, 0, 2, 2), (1, 2, 1), 256, 65536, "C")]
    # top_wm != 4: the caller's pin of 256-row blocks does nothing - the plan is the unpinned one (144 tiles: 128-row blocks)
    pinned, free, off = (one(f"M=1536 N=3072 K=1024 epi=4 epi_rows=1536 {x}") for x in ("force_wm=4", "", "force_wm=4 sw.top_wm=0"))
    assert _launches(off) == _launches(free) == [(0, 1536, (0, 2, 2, 0, 2, 2), (24, 12, 1), 256, 65536, "S")] != _launches(pinned)
    assert [l["tile_band"] for l in one("M=24576 N=5504 K=1024 epi=2 sw.band=8")["launches"]] == [8, 8]
    assert [l["tile_band"] for l in one("M=24576 N=5504 K=1024 epi=2")["launches"]] == [4, 4]
    # rpf = 0: no residual prefetch, and its sink (4096) and line buffer (2048) leave the LDS size
    for c, on, off in zip(RESIDUAL_CASES, dump(RESIDUAL_CASES)[0], dump([c + " sw.rpf=0" for c in RESIDUAL_CASES])[0]):
        assert all(l["r_prefetch"] == 1 for l in on["launches"]) and all(l["r_prefetch"] == 0 for l in off["launches"]), c
        gsums = "ln_in_gsums" in c   # (the folded LayerNorm's group sums keep both buffers)
        assert [l["lds"] for l in off["launches"]] == [l["lds"] - (0 if gsums else 6144) for l in on["launches"]], c
        assert [_key(l) for l in off["launches"]] == [_key(l) for l in on["launches"]], c
    assert all(l["row_major_epi"] == 1 for r in dump(cases)[0] for l in r["launches"])
    assert all(l["row_major_epi"] == 0 for r in dump([c + " sw.rme=0" for c in cases])[0] for l in r["launches"])


def test_stream_k(dump):
    sk = "sk_ws=1 sk_force=1"
    (a, b, no_xcd, bias_m, ksplit, plain_b, plain_k), _ = dump([
        f"M=1536 N=3072 K=1024 {sk}", f"M=100 N=100 K=64 {sk}", f"M=1536 N=3072 K=1024 {sk} xcd=0", f"M=1536 N=3072 K=1024 {sk} bias_m=1",
        f"M=1536 N=3072 K=1024 {sk} ksplit=2 kpart=1", "M=1536 N=3072 K=1024 bias_m=1", "M=1536 N=3072 K=1024 ksplit=2 kpart=1"])
    (l,) = a["launches"]
    assert (l["sk"], l["sk_tiles"], l["grid"], l["threads"], l["lds"], l["prof"], l["tile_band"], l["in_table"]) == (1, 144, [256, 1, 1], 512, 151552, "S", 0, 1) and a["xcd_calls"] == 1
    assert l["lds"] == l["lds_max"] and l["variant"] == [0, 4, 3, 0, 2, 2]
    (l,) = b["launches"]
    assert (l["sk"], l["sk_tiles"], l["grid"]) == (1, 1, [8, 1, 1])
    free = _launches(dump(["M=1536 N=3072 K=1024"])[0][0])
    assert _launches(no_xcd) == free and no_xcd["xcd_calls"] == 1
    assert _launches(bias_m) == _launches(plain_b) and bias_m["xcd_calls"] == 0      # the probe is asked last
    assert _launches(ksplit) == _launches(plain_k) and ksplit["xcd_calls"] == 0
    # switch 1 routes by gemm_sk_pays (144 tiles: 44 % of the round empty -> pays; 2304 tiles: 9 whole rounds -> does not), 2 takes every problem with a workspace
    pays, not_pays, always = dump(["M=1536 N=3072 K=1024 sk_ws=1 sw.sk=1", "M=24576 N=3072 K=1024 sk_ws=1 sw.sk=1", "M=24576 N=3072 K=1024 sk_ws=1 sw.sk=2"])[0]
    assert [r["launches"][0]["sk"] for r in (pays, not_pays, always)] == [1, 0, 1]
    # default switches and no per-call force: the probe is never asked, workspace or not
    res, _ = dump([c + " sk_ws=1" for c in EXPECTED])
    assert all(r["xcd_calls"] == 0 for r in res)
    assert [_launches(r) for r in res] == list(EXPECTED.values())


def test_invariants_over_a_sweep(dump):
    Ms, Ns, Ks = [1, 64, 127, 128, 129, 255, 256, 257, 1536, 3072, 8485, 24576], [4, 100, 128, 136, 1024, 3072, 5504], [32, 96, 1024]
    sweep = list(itertools.product(Ms, Ns, Ks, [1, 2, 3], [0, 1]))
    res, table = dump([f"M={m} N={n} K={k} ksplit={s} w16={w} kpart={int(s > 1)}" for (m, n, k, s, w) in sweep])
    planned = two = 0
    for (m, n, k, s, w), r in zip(sweep, res):
        if "error" in r:
            assert s > 1 and "split-K needs" in r["error"], ((m, n, k, s, w), r)   # (the only refusal these arguments can meet)
            continue
        planned += 1
        ls = r["launches"]
        for l in ls:
            mode, wm, st, ks, ti, tj = l["variant"]
            assert l["in_table"] == 1 and _key(l) in table, l
            assert l["w16"] == w and l["lds"] <= l["lds_max"] <= 160 * 1024, l
            assert l["threads"] == wm * 512 // (ti * tj), l
            rows = l["rows"][1] - l["rows"][0]
            assert rows > 0 and l["grid"][0] == -(-n // 128) and l["grid"][1] * wm * 64 >= rows > (l["grid"][1] - 1) * wm * 64 and l["grid"][2] == s, l
            assert l["reduce"] == int(s > 1) and ks == int(s > 1), l
            assert l["work"] == 2.0 * rows * n * k, l
        assert ls[0]["rows"][0] == 0 and ls[-1]["rows"][1] == m, ls
        if len(ls) == 2:
            two += 1
            cut = ls[0]["rows"][1]
            assert ls[1]["rows"][0] == cut and 0 < cut < m and cut % 256 == 0, ls
            assert (ls[0]["no_row_split"], ls[0]["force_wm"], ls[1]["no_row_split"], ls[1]["force_wm"]) == (1, 4, 1, 0), ls
            assert ls[0]["variant"][:3] == [0, 4, 3], ls
    assert planned > len(sweep) // 2 and two >= 8, (planned, two)
    # a row range that does not start at 0 (the caller's own m_base) is tiled the same way
    # (91 row tiles x 43 = 3913 tiles = 15 rounds + 73: 89 row tiles fill the whole rounds, 2 are left)
    (r,), _ = dump(["M=24576 N=5504 K=1024 m_base=1280"])
    assert _launches(r) == [(1280, 24064, (0, 4, 3, 0, 2, 2), (43, 89, 1), 512, 147456, "G"), (24064, 24576, (0, 2, 4, 0, 1, 2), (43, 4, 1), 512, 131072, "S")]


REFUSALS = {
    "conv=1 n=1 h=16 w=16 cin=48 N=128": "conv3x3: Cin=48 must be a multiple of 32",
    "conv=1 n=1024 h=64 w=64 cin=256 N=128": "conv3x3 (LDS-DMA): the activation planes (4294967296 bytes) must stay below 4 GiB per launch",
    "M=128 N=128 K=32 A_hi=0": "gemm_split_glds: both operands must be pre-split",
    "conv=1 n=1 h=16 w=8 cin=128 N=128 gn_part=1": "gemm_split_glds: GroupNorm partials need whole 256 x 128 tiles of a convolution with the plain epilogue (M=128 N=128)",
    "M=128 N=128 K=48": "gemm_split_glds: K, lda, ldb must be multiples of 32 (K=48 lda=48 ldb=48)",
    "M=128 N=128 K=32 batch=2": "gemm_split_glds: batched form not provided",
    "M=1536 N=2048 K=1024 epi=3 R=1": "gemm_split_glds: bad fused k/v-preparation arguments",
    "M=1536 N=100 K=1024 epi=2": "gemm_split_glds: bad fused GEGLU arguments (N=100 ldc=100)",
    "M=1536 N=3072 K=1024 epi=4 ksplit=2 kpart=1": "gemm_split_glds: bad fused q/k/v-preparation arguments",
    "M=1536 N=1024 K=1024 epi=1 bias_n=1": "gemm_split_glds: bad fused q-preparation arguments",
    "M=1536 N=1024 K=1024 ln_in_stats=1 ksplit=2 kpart=1": "gemm_split_glds: bad folded-LayerNorm consumer arguments (N=1024 ksplit=2 groups=32)",
    "M=1536 N=1024 K=1024 ln_out=1 ln_out_ld=48": "gemm_split_glds: bad folded-LayerNorm producer arguments (ld=48 N=1024 epi=0)",
    "M=1536 N=1024 K=1024 epi=1 ksplit=2 kpart=1": "gemm_split_glds: split-K needs a workspace, the plain epilogue, the 128-row tile and >= 2 k-tiles per slice (ksplit=2 K=1024)",
}


def test_refusals(dump):
    res, _ = dump(list(REFUSALS))
    for (c, msg), r in zip(REFUSALS.items(), res):
        assert r.get("error") == msg, (c, r)
