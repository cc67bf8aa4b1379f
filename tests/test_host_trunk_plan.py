"""CPU checks of the launch plans of the I3D and Inception-v3 trunks (csrc/i2v_trunk_plan.h).  tests/trunk_plan_host_check.cpp, a
stand-alone host program, prints every step of every plan with all its fields, the sizes, offsets and refusals; this module compares
them (a) with the shapes the project's own torch modules produce when their conv layers are run on the CPU, (b) with
tests/golden/trunk_plan_parent.json, recorded from the launches and size queries of the code before the plans existed, and (c) checks
that a perturbed plan is counted.  The program is also built with AddressSanitizer and UBSan and run directly."""
import json
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import fid_common as fc
import i3d_units_common as uc
from conftest import PKG, REPO
from metrics.DTFVD import ID3, ID3_32
from metrics.FID import inception as inc_mod
from metrics.PyTorch_FVD import I3D as kin_mod

SRC = os.path.join(REPO, "tests", "trunk_plan_host_check.cpp")
STEP = re.compile(r"  (\w+) u=(-?\d+) blk=(-?\d+) pool=(-?\d+) (\S+)->(\S+) in=([\d,]+) out=([\d,]+) k=([\d,]+) s=([\d,]+) p=([\d,]+) e=([\d,]+) "
                  r"cs=(\d+)\+(\d+)->(\d+)\+(\d+) C=(\d+) relu=(\d) chw=(\d) grid=(\d+) nt=(\d)$")


def build(tmp, san):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp / ("check_san" if san else "check")
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if san else ["-O1"]
    r = subprocess.run([hipcc, "-std=c++17", "-Wall", "-Werror", "--offload-arch=gfx950"] + flags + ["-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(REPO, "include"),
                        "-x", "hip", SRC, "-o", str(exe)], capture_output=True, text=True, timeout=900)
    if san and r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libclang_rt\.\w+san", r.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(exe, *args):
    out = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-2000:]
    cases, cur = {}, None
    for line in out.stdout.splitlines():
        if line.startswith("case "):
            cur = cases.setdefault(line[5:], {"lines": []})
            cur["lines"].clear()
        elif line.startswith("digest "):
            _, cid, digest, _, n = line.split()
            assert cases[cid] is cur and int(n) == len(cur["lines"])
            cur["digest"], cur = digest, None
        elif cur is not None:
            cur["lines"].append(line)
    return cases, out.stdout


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = build(tmp_path_factory.mktemp("trunk_plan"), False)
    cases, text = run(exe)
    return {"exe": exe, "cases": cases, "text": text}


def steps(case):
    out = []
    for line in case["lines"]:
        m = STEP.match(line)
        if m:
            g = m.groups()
            t3 = lambda s: tuple(int(v) for v in s.split(","))  # noqa: E731
            out.append({"kind": g[0], "unit": int(g[1]), "blk": int(g[2]), "pool": int(g[3]), "src": g[4], "dst": g[5], "in": t3(g[6]), "out": t3(g[7]),
                        "k": t3(g[8]), "s": t3(g[9]), "p": t3(g[10]), "e": t3(g[11]), "ics": int(g[12]), "ioff": int(g[13]), "ocs": int(g[14]),
                        "ooff": int(g[15]), "C": int(g[16]), "relu": int(g[17]), "chw": int(g[18]), "grid": int(g[19]), "nt": int(g[20])})
        else:
            assert not line.startswith("  "), line
    return out


# ---------------------------------------------------------------------------------------------------------------- (b), (c), sanitizers

def test_every_plan_equals_the_launches_of_the_code_before_the_plans(plans):
    """Case by case against tests/golden/trunk_plan_parent.json: the three I3D variants (logits and features, B 1 and 3, T 8 .. 32 with
    the refusals at 8 and 24), Inception at 36 maps with all taps and at five maps x last 0..3 x B 1, 3 x taps none / all / block 2
    (side 74: refused by the entries, inc_dims_ok), and every sub-module builder at the shapes of i3d_units_common and fid_common.  A
    digest covers every launch's kind, unit, buffers, maps, window, stride, padding, channel slices, grid and tile, and every size."""
    want = json.load(open(os.path.join(REPO, "tests", "golden", "trunk_plan_parent.json")))["cases"]
    got = plans["cases"]
    assert set(got) == set(want) and len(want) == 500
    bad = {k: (got[k]["digest"], len(got[k]["lines"]), v) for k, v in want.items() if (got[k]["digest"], len(got[k]["lines"])) != (v["digest"], v["lines"])}
    assert not bad, bad
    for v, t in (("kin", 8), ("dt16", 8), ("dt32", 24)):
        for mode in ("logits", "features"):
            for b in (1, 3):
                head = got[f"i3d/{v}/{mode}/B{b}/T{t}"]["lines"]
                assert head[0].startswith(f"refused code=-1 msg=i3d: {t} frames leave a [") and head[1] == "bytes=0 t_head=0" and len(head) == 2
    assert got["i3d/kin/logits/B1/T9"]["lines"][0].endswith("t_head=1") and got["i3d/dt32/features/B3/T32"]["lines"][0].endswith("t_head=1")
    assert got["i3d/dt16/features/B1/T32"]["lines"][0].endswith("t_head=3")
    assert all(c["lines"][0].startswith("dims_ok=0 ") for k, c in got.items() if k.startswith("inception/74x74/"))
    assert all(c["lines"][0].startswith("dims_ok=1 ") for k, c in got.items() if k.startswith("inception/75x80/"))
    assert got["inc_mixed/b3/B1/1x1"]["lines"] == ["refused code=-1 msg=inception Mixed_6a.branch3x3: a [1, 1] map is too small"]
    # the slot sizes do not depend on the taps
    for last in range(4):
        sizes = {t: got[f"inception/128x299/last{last}/B3/taps{t}"]["lines"][:2] for t in ("0", "f", "4")}
        assert sizes["0"] == sizes["f"] == sizes["4"]


def test_a_perturbed_plan_is_counted(plans):
    """--perturb: the front pad of the strided I3D unit of every plan that has one, else the channel offset of the first concatenation
    slice, is changed before printing.  Every whole-trunk plan that reaches such a step must then miss its digest."""
    want = json.load(open(os.path.join(REPO, "tests", "golden", "trunk_plan_parent.json")))["cases"]
    got, _ = run(plans["exe"], "--perturb")
    missed = {k for k, v in want.items() if got[k]["digest"] != v["digest"]}
    for k, c in plans["cases"].items():
        has = any(s["kind"] == "conv" and (s["s"][0] > 1 or s["ooff"] > 0) for s in steps(c))
        assert (k in missed) == has, k
    assert len(missed) > 300
    assert sum(k.startswith("i3d/") for k in missed) == 3 * 2 * 2 * 8 - 32 and sum(k.startswith("inception/") for k in missed) == 36 + 5 * 2 * 2 * 3 - 4   # last >= 2; four ids occur in both lists


def test_sanitizer_build_prints_the_same(plans, tmp_path):
    """The check program built stand-alone with -fsanitize=address,undefined -fno-sanitize-recover=all and run directly."""
    _, text = run(build(tmp_path, True))
    assert text == plans["text"]


# ---------------------------------------------------------------------------------------------------------------- (a) torch modules

def hooked(net, kind):
    """Forward hooks on every conv layer of a holder module: (module name, input shape, output shape) in call order."""
    seen = []
    for name, m in net.named_modules():
        if isinstance(m, kind):
            m.register_forward_hook(lambda mod, inp, out, name=name: seen.append((name, tuple(inp[0].shape), tuple(out.shape))))
    return seen


I3D_NETS = {"kin": (lambda: kin_mod.I3D(400), "kin", 2), "dt16": (lambda: ID3.InceptionI3D(18), "dt", 2), "dt32": (lambda: ID3_32.InceptionI3D(18), "dt", 4)}


@pytest.mark.parametrize("name,T", [("kin", 9), ("kin", 17), ("dt16", 9), ("dt16", 17), ("dt32", 25), ("dt32", 32)])
def test_i3d_plan_has_the_shapes_of_the_torch_module(plans, name, T):
    """The module's own Conv3d layers (hooked) run on 1 x 3 x T x 224 x 224 behind explicit SAME padding (i3d_units_common.same_pads,
    written from the layer definitions), the zero-padded ceil-mode max pools and torch.cat: every step's maps and channels, and every
    concatenation's offsets and total, are the plan's."""
    make, variant, pool_t = I3D_NETS[name]
    torch.manual_seed(0)
    net = make().eval()
    seen = hooked(net, torch.nn.Conv3d)
    dt = variant == "dt"
    cap = (lambda s: s[0].upper() + s[1:]) if dt else (lambda s: s)
    events = []

    def unit(mod, index, x):
        y = mod.conv3d(uc._pad(x, uc.same_pads(variant, mod.conv3d.kernel_size, mod.conv3d.stride, x.shape[2:])))
        events.append(("conv", index, tuple(x.shape[2:]), seen[-1][2][2:], seen[-1][2][1]))
        return y

    def pool(x, kernel, stride):
        y = uc.maxpool_oracle(variant, x, kernel, stride)
        events.append(("i3dpool", -1, tuple(x.shape[2:]), tuple(y.shape[2:]), y.shape[1]))
        return y

    with torch.no_grad():
        x = torch.randn(1, 3, T, 224, 224)
        x = unit(getattr(net, cap("conv3d_1a_7x7")), 0, x)
        x = pool(x, (1, 3, 3), (1, 2, 2))
        x = unit(getattr(net, cap("conv3d_2b_1x1")), 1, x)
        x = unit(getattr(net, cap("conv3d_2c_3x3")), 2, x)
        x = pool(x, (1, 3, 3), (1, 2, 2))
        cats = []
        for i, (mname, _cin, _o) in enumerate(kin_mod.MIXED):
            m = getattr(net, cap(mname))
            br = [m.b0, m.b1a, m.b1b, m.b2a, m.b2b, m.b3b] if dt else [m.branch_0, m.branch_1[0], m.branch_1[1], m.branch_2[0], m.branch_2[1], m.branch_3[1]]
            u = 3 + 6 * i
            y0 = unit(br[0], u, x)
            y1 = unit(br[2], u + 2, unit(br[1], u + 1, x))
            y2 = unit(br[4], u + 4, unit(br[3], u + 3, x))
            y3 = unit(br[5], u + 5, pool(x, (3, 3, 3), (1, 1, 1)))
            x = torch.cat((y0, y1, y2, y3), 1)
            cats.append(([0, y0.shape[1], y0.shape[1] + y1.shape[1], y0.shape[1] + y1.shape[1] + y2.shape[1]], x.shape[1]))
            if i == 1:
                x = pool(x, (3, 3, 3), (2, 2, 2))
            if i == 6:
                x = pool(x, (2, 2, 2), (2, 2, 2))
        pooled = F.avg_pool3d(x, (pool_t, 7, 7), stride=1)
        events.append(("avgpool", -1, tuple(x.shape[2:]), tuple(pooled.shape[2:]), pooled.shape[1]))
    assert len(seen) == 57 and [e[1] for e in events if e[0] == "conv"] == list(range(57))
    got = steps(plans["cases"][f"i3d/{name}/features/B1/T{T}"])
    assert got[0]["kind"] == "input" and got[0]["out"] == (T, 224, 224)
    assert [(s["kind"], s["unit"], s["in"], s["out"], s["C"]) for s in got[1:]] == events
    for i, (offs, total) in enumerate(cats):
        finals = [s for s in got if s["kind"] == "conv" and s["unit"] in (3 + 6 * i, 5 + 6 * i, 7 + 6 * i, 8 + 6 * i)]
        assert [s["ooff"] for s in finals] == offs and {s["ocs"] for s in finals} == {total} and len({s["dst"] for s in finals}) == 1
    # the logits plan: the same trunk, then the classifier on the pooled map and the time mean
    logits = steps(plans["cases"][f"i3d/{name}/logits/B1/T{T}"])
    assert [(s["kind"], s["in"], s["out"]) for s in logits[1:len(got)]] == [(s["kind"], s["in"], s["out"]) for s in got[1:]]
    assert [(s["kind"], s["unit"], s["in"], s["C"]) for s in logits[len(got):]] == [("conv", 57, tuple(pooled.shape[2:]), net.state_dict()[
        ("logits" if dt else "conv3d_0c_1x1") + ".conv3d.weight"].shape[0]), ("timemean", -1, tuple(pooled.shape[2:]), 400 if not dt else 18)]


@pytest.mark.parametrize("hw", [(75, 80), (299, 299)])
def test_inception_plan_has_the_shapes_of_the_torch_module(plans, hw):
    """The holder's own Conv2d layers (hooked; they carry kernel, stride and padding) in the graph of fid_common.block_branches, the
    three pools as torch states them and the concatenation: every step's unit, maps and channels and every slice's offset and total."""
    torch.manual_seed(0)
    net = inc_mod.InceptionV3(output_blocks=[0, 1, 2, 3])
    seen = hooked(net, torch.nn.Conv2d)
    events = []

    def conv(key, blk, index, x, off, total):
        y = net.get_submodule(key).conv(x)
        assert seen[-1][0] == key + ".conv"
        events.append(("conv", blk, index, seen[-1][1][2:], seen[-1][2][2:], seen[-1][2][1], off, total))
        return y

    def pool(kind, x, off, total):
        y = F.max_pool2d(x, 3, 2) if kind == fc.POOL_MAX_S2 else F.max_pool2d(x, 3, 1, 1) if kind == fc.POOL_MAX_S1 else \
            F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)
        events.append(("incpool", -1, kind, tuple(x.shape[2:]), tuple(y.shape[2:]), y.shape[1], off, total))
        return y

    blocks = {}
    with torch.no_grad():
        x = torch.randn(1, 3, *hw)
        for j, u in enumerate(fc.STEM):
            x = conv(u[0], -1, j, x, 0, u[2])
            if j in (2, 4):
                x = pool(fc.POOL_MAX_S2, x, 0, x.shape[1])
                blocks[j // 2 - 1] = x.shape
        for i, (bname, kind, cin, par) in enumerate(fc.MIXED):
            names = list(fc.block_units(kind, cin, par))
            total = sum((fc.block_units(kind, cin, par)[s][1] if isinstance(s, str) else cin) for _, lasts in fc.block_branches(kind, par) for s in lasts)
            outs, off = [], 0
            for front, lasts in fc.block_branches(kind, par):
                h = x
                for s in front:
                    h = conv(f"{bname}.{s}", i, names.index(s), h, 0, None) if isinstance(s, str) else pool(s, h, 0, None)
                for s in lasts:
                    outs.append(conv(f"{bname}.{s}", i, names.index(s), h, off, total) if isinstance(s, str) else pool(s, h, off, total))
                    off += outs[-1].shape[1]
            x = torch.cat(outs, 1)
            assert x.shape[1] == total
            if i == 7:
                blocks[2] = x.shape
    assert len(seen) == 94
    case = plans["cases"][f"inception/{hw[0]}x{hw[1]}/last3/B1/tapsf"]
    got = steps(case)
    want = [(e[0], e[1], e[2], (1, *e[3]), (1, *e[4]), e[5], e[6]) for e in events]
    assert [(s["kind"], s["blk"], s["unit"] if s["kind"] == "conv" else s["pool"], s["in"], s["out"], s["C"], s["ooff"]) for s in got[:-1]] == want
    for s, e in zip(got, events):
        assert s["ocs"] == (e[7] if e[7] is not None else e[5])
    assert got[-1]["kind"] == "globalavg" and got[-1]["in"] == (1, 1, x.shape[2] * x.shape[3]) and got[-1]["C"] == 2048 and got[-1]["dst"] == "tap3"
    shapes = {int(m.group(1)): tuple(int(v) for v in m.group(2).split(",")) for m in (re.match(r"block(\d)=([\d,]+)", ln) for ln in case["lines"]) if m}
    assert shapes == {0: (*blocks[0][2:], 64), 1: (*blocks[1][2:], 192), 2: (*blocks[2][2:], 768), 3: (1, 1, 2048)}
