"""The shape of a Route A decode step (bevgen_amd/csrc/ar_plan.h) on the CPU: effective path, fused or per-operator step, chains, the fused MLP launch, the split layer's
key walk, the pick launch's tail, and the G that ar_prefill asks with.

tests/host/ar_plan_dump.cpp is built for the host only, with the address and undefined-behaviour sanitizers, and run directly: no GPU and no HIP call.  The expected
decisions are for config 4 (D = 1024, H = 16, V = 1024, K = 256, L = 2368; 256 CUs, XCD placement verified); they were derived by hand from the driver these functions
were taken out of and confirmed against a copy of its own rule code over a grid of inputs (experiments/r18.md)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

FUSED, PER_OP, SPLIT, AUTO = range(4)   # BEVGEN_DECODE_*


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ar_plan") / "ar_plan_dump")
    r = subprocess.run([HIPCC, "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", os.path.join(ROOT, "bevgen_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined",
                        os.path.join(ROOT, "tests", "host", "ar_plan_dump.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        """one process for all `cases`; returns one result per case"""
        p = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])   # (a sanitizer report goes to stderr)
        out = [json.loads(line) for line in p.stdout.splitlines()]
        assert len(out) == len(cases) and not any("error" in o for o in out), out
        return out

    return run


def _case(fn, **kw):
    return fn + " " + " ".join(f"{k.replace('__', '.')}={v}" for k, v in kw.items())


def _plan(**kw):
    return _case("plan", **kw)


def test_shape_predicates(dump):
    got = dump(["ksplit N=1024 K=4096", "ksplit N=4096 K=1024", "ksplit N=1024 K=1024", "splits B=1 H=16 L=2368", "lds G=1", "lds G=4"])
    assert [list(g.values())[0] for g in got] == [4, 1, 4, 8, 24188, 51644]   # (both LDS needs fit the 64 KiB the plan allows)


def test_auto_path_fp32_weights_splits_up_to_four_sequences(dump):
    got = dump([_plan(B=b) for b in (1, 2, 3, 4, 6, 8, 16)])
    assert [(g["path"], g["fused"], g["split"]) for g in got] == [(SPLIT, 1, 1)] * 4 + [(FUSED, 1, 0)] * 3
    assert [g["needs_split_qkv_image"] for g in got] == [1, 1, 1, 1, 0, 0, 0]


def test_auto_path_counts_layout_groups_and_prefill_asks_with_the_group_size_only_where_the_fused_step_holds(dump):
    grouped, alone, odd_prefix, per_op = dump([_case("prefill", B=8, S=2), _plan(B=8, G=1), _case("prefill", B=8, S=2, K=250), _case("prefill", B=8, S=2, path=PER_OP)])
    # eight sequences in groups of two are four sequences per group: the split layer, with G = S
    assert (grouped["G"], grouped["path"], grouped["fused"], grouped["split"], grouped["needs_split_qkv_image"]) == (2, SPLIT, 1, 1, 1)
    assert (alone["path"], alone["split"]) == (FUSED, 0)
    # a shared prefix that does not end on a 16-key boundary, or the per-operator path: the prefix is replicated, G = 1
    assert (odd_prefix["G"], odd_prefix["path"], odd_prefix["fused"]) == (1, FUSED, 1)
    assert (per_op["G"], per_op["path"], per_op["fused"]) == (1, PER_OP, 0)


def test_auto_path_fp16_weights_is_fused_at_every_batch_size_while_the_fused_mlp_launch_is_ready(dump):
    ready = dump([_plan(B=b, wf16=1) for b in range(1, 65)])
    assert all((g["path"], g["fused"], g["split"], g["mlp_fused"]) == (FUSED, 1, 0, 1) for g in ready)
    fp32_rule = dump([_plan(B=b, wf16=1, ready=0) for b in (1, 2, 3, 4, 6, 8, 16)])
    assert [g["path"] for g in fp32_rule] == [SPLIT] * 4 + [FUSED] * 3 and not any(g["mlp_fused"] for g in fp32_rule)
    # ... and with shared-prefix groups (G > 1) the fp32 rule as well
    assert dump([_plan(B=8, G=2, wf16=1)])[0]["path"] == SPLIT


def test_more_than_64_sequences_take_the_per_operator_step(dump):
    for g in dump([_plan(B=65), _plan(B=65, path=FUSED), _plan(B=65, path=SPLIT, chains=4), _plan(B=65, wf16=1)]):
        assert (g["fused"], g["split"], g["chains"], g["Bc"], g["mlp_fused"], g["pick_embeds"], g["attn_ksplit"]) == (0, 0, 1, 65, 0, 0, 1), g
    assert dump([_plan(B=65, path=SPLIT)])[0]["needs_split_qkv_image"] == 1   # (the configured path still asks for its operand image)
    assert dump([_plan(B=4, path=PER_OP)])[0]["fused"] == 0


def test_split_layer_key_walk(dump):
    got = dump([_plan(B=1), _plan(B=2), _plan(B=4), _plan(B=8, path=SPLIT), _plan(B=4, path=SPLIT, chains=2), _plan(B=4, G=2, path=SPLIT), _plan(B=1, path=FUSED)])
    #                                    1    2    4    8: 128 (sequence, head) pairs   two chains of two   shared prefix   not the split layer
    assert [g["attn_ksplit"] for g in got] == [4, 4, 2, 1, 4, 1, 1]


def test_fused_mlp_launch(dump):
    on = dump([_plan(B=b, path=FUSED) for b in (1, 16, 64)])
    assert all(g["mlp_fused"] == 1 and g["down_ksplit"] == 4 and g["ln2_fold"] == 1 for g in on)
    off = dump([_plan(B=16, path=FUSED, chains=2), _plan(B=16, path=FUSED, sw__ln2_fold=0), _plan(B=16, path=FUSED, sw__mlp_fuse=0), _plan(B=16, path=FUSED, ready=0),
                _plan(B=16, path=FUSED, cus=128), _plan(B=16, path=FUSED, placement=0), _plan(B=16, path=FUSED, D=256, H=4, V=64, K=16, L=48), _plan(B=4, path=SPLIT)])
    assert [g["mlp_fused"] for g in off] == [0] * 8 and all(g["fused"] == 1 for g in off)
    assert off[1]["ln2_fold"] == 0 and off[6]["down_ksplit"] == 4   # (the tiny model: four K slices of 256 all the same; it is the width that rules the launch out)


def test_pick_tail(dump):
    got = dump([_plan(B=16, path=FUSED), _plan(B=4), _plan(B=16, path=FUSED, sw__pick_tail=0), _plan(B=16, path=FUSED, chains=2), _plan(B=16, path=PER_OP), _plan(B=65)])
    assert [g["pick_embeds"] for g in got] == [1, 1, 0, 0, 0, 0]


def test_chains(dump):
    got = dump([_plan(B=16, path=FUSED, chains=c) for c in (0, 1, 2, 3, 4, 9)] + [_plan(B=6, path=FUSED, chains=4), _plan(B=12, G=2, path=FUSED, chains=4),
                                                                                  _plan(B=16, path=FUSED, chains=4, trace=1), _plan(B=7, path=FUSED, chains=4)])
    assert [(g["chains"], g["Bc"]) for g in got] == [(1, 16), (1, 16), (2, 8), (2, 8), (4, 4), (4, 4), (3, 2), (3, 4), (1, 16), (1, 7)]


def test_graph_replay_rule(dump):
    got = dump(["graph steps=3", "graph steps=2", "graph steps=100 logits=1", "graph steps=100 prof=1", "graph steps=100 off=1"])
    assert [g["graph"] for g in got] == [1, 0, 0, 0, 0]
