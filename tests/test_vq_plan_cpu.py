"""The pure part of the VQGAN host driver (bevgen_amd/csrc/vq_plan.h) on the CPU: activation sizes, the pass cut, the range-safe sites of a pass and the upsample form.

tests/host/vq_plan_dump.cpp is built for the host only, with the address and undefined-behaviour sanitizers, and run directly: no GPU and no HIP call.  The expected values
are for the released f16 VQGAN (ch 128, ch_mult [1, 1, 2, 2, 4], two res blocks, attention at 16, resolution 256); they were derived by hand from the driver these functions
were taken out of and confirmed against a copy of its own scan, count and rule code (experiments/r14.md)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

PLANES, RANGED_F32, PLAIN = range(3)   # VqUpForm


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vq_plan") / "vq_plan_dump")
    r = subprocess.run([HIPCC, "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", os.path.join(ROOT, "bevgen_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined",
                        os.path.join(ROOT, "tests", "host", "vq_plan_dump.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        """one process for all `cases`; returns one result per case"""
        p = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])   # (a sanitizer report goes to stderr)
        out = [json.loads(line) for line in p.stdout.splitlines()]
        assert len(out) == len(cases) and not any("error" in o for o in out), out
        return out

    return run


def _shape(encoder, ch=128, ch_mult=(1, 1, 2, 2, 4), res_blocks=2, resolution=256, attn_resolution=16, in_channels=3):
    """the shape vq_finalize / vq_enc_finalize fill for a checkpoint of the reference model (stage1/model.py: a block has a nin_shortcut where its channels change)"""
    levels = len(ch_mult)
    nin, first, attn = [0] * levels, [0] * levels, [0] * levels
    for lvl in range(levels):
        if encoder:
            block_in, res = ch * ((1,) + tuple(ch_mult))[lvl], resolution >> lvl
        else:
            block_in, res = ch * ch_mult[min(lvl + 1, levels - 1)], resolution >> lvl
        changes = int(block_in != ch * ch_mult[lvl])   # only the level's first block can change the channels
        nin[lvl], first[lvl], attn[lvl] = changes, changes, int(res == attn_resolution)
    resample = [int(lvl != levels - 1) for lvl in range(levels)] if encoder else [int(lvl != 0) for lvl in range(levels)]
    lst = lambda v: ",".join(str(x) for x in v)
    return (f"encoder={int(encoder)} levels={levels} ch={ch} ch_mult={lst(ch_mult)} attn={lst(attn)} nin={lst(nin)} first_nin={lst(first)} resample={lst(resample)} mid_nin=0 "
            f"cin_pad={(in_channels + 31) // 32 * 32 if encoder else 0}")


DEC, ENC = _shape(False), _shape(True)


def test_released_decoder_sizes(dump):
    square, rect = dump([f"scan {DEC} h=16 w=16", f"scan {DEC} h=14 w=25"])
    assert square == {"per_img": 8388608, "max_c": 512, "attn_hw": 256, "attn_hwp": 256, "lat": [16, 16], "image": [256, 256]}
    assert rect == {"per_img": 11468800, "max_c": 512, "attn_hw": 350, "attn_hwp": 352, "lat": [14, 25], "image": [224, 400]}


def test_released_encoder_sizes(dump):
    assert "cin_pad=32" in ENC
    square, rect = dump([f"scan {ENC} h=256 w=256", f"scan {ENC} h=224 w=400"])
    assert square == {"per_img": 8388608, "max_c": 512, "attn_hw": 256, "attn_hwp": 256, "lat": [16, 16], "image": [256, 256]}
    assert (rect["lat"], rect["attn_hw"], rect["attn_hwp"], rect["image"]) == ([14, 25], 350, 352, [224, 400])


def test_pass_cut(dump):
    n96, n50, n1, n48, n49 = dump([f"cut n={n}" for n in (96, 50, 1, 48, 49)])
    assert n96 == {"chunk": 48, "passes": 2, "images": [48, 48]}
    assert n50 == {"chunk": 48, "passes": 2, "images": [48, 2]}
    assert n1 == {"chunk": 1, "passes": 1, "images": [1]}
    assert n48 == {"chunk": 48, "passes": 1, "images": [48]} and n49 == {"chunk": 48, "passes": 2, "images": [48, 1]}


def test_sites_per_pass(dump):
    dec, enc = dump([f"sites {DEC}", f"sites {ENC}"])
    assert dec == {"per_pass": 7, "feeds_nin": [0, 0, 0, 0, 0]}   # conv_in, 2 nin_shortcuts, 4 upsamples: 14 per call of 96 images
    assert enc == {"per_pass": 8, "feeds_nin": [0, 1, 0, 1, 0]}   # conv_in, quant_conv, 2 nin_shortcuts, 4 downsamples: 16; levels 2 and 4 open with a nin_shortcut
    assert dec["per_pass"] * dump(["cut n=96"])[0]["passes"] == 14 and enc["per_pass"] * dump(["cut n=96"])[0]["passes"] == 16
    # the mid blocks count too, and a level that does not resample feeds nothing
    odd = dump([f"sites encoder=1 levels=2 ch=32 ch_mult=1,2 nin=0,2 first_nin=0,1 resample=1,0 mid_nin=1 cin_pad=32",
                f"sites encoder=1 levels=2 ch=32 ch_mult=1,2 nin=0,1 first_nin=0,0 resample=1,0 mid_nin=0 cin_pad=32"])
    assert odd == [{"per_pass": 6, "feeds_nin": [1, 0]}, {"per_pass": 4, "feeds_nin": [0, 0]}]


def test_upsample_form(dump):
    up = lambda C, **kw: f"up C={C} " + " ".join(f"{k.replace('__', '.')}={v}" for k, v in kw.items())
    forms = lambda cases: [r["form"] for r in dump(cases)]
    # split precision: planes where C / 4 is a power of two and C % 32 == 0, with or without the range-safe mode
    assert forms([up(C, planes=1, range=r) for C in (512, 256, 128) for r in (0, 1)]) == [PLANES] * 6
    assert forms([up(C, planes=1, range=r) for C in (96, 48) for r in (0, 1)]) == [PLAIN, RANGED_F32, PLAIN, RANGED_F32]   # C / 4 = 24 | 12
    # the planes switch off: ranged fp32 under vq_range, else plain
    assert forms([up(C, planes=1, range=r, sw__up_planes=0) for C in (512, 96) for r in (0, 1)]) == [PLAIN, RANGED_F32, PLAIN, RANGED_F32]
    # fp32 precision: always plain
    assert forms([up(C, planes=0, range=r, sw__up_planes=s) for C in (512, 96) for r in (0, 1) for s in (0, 1)]) == [PLAIN] * 8
