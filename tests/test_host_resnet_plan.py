"""CPU checks of the launch plans of the motion encoder and the conditioning embedder (csrc/i2v_resnet_plan.h).
tests/resnet_plan_host_check.cpp, a stand-alone host program, prints every step of every plan with all its fields, the sizes, offsets
and refusals; this module compares them (a) with tests/golden/resnet_plan_parent.json, recorded from the launches and size queries of
the code before the plans existed, (b) checks that a perturbed plan is counted, (c) walks every plan for slot liveness, (d) compares
the conv steps with the convs of the float64 oracles and the forms with tests/encoder_cfgs.py::encoder_paths.  (e) The program is also
built with AddressSanitizer and UBSan and run directly."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_cfgs as ec
import i2v_synth as synth
from conftest import PKG, REPO
from oracle import embedder_ref, encoder_ref

SRC = os.path.join(REPO, "tests", "resnet_plan_host_check.cpp")
GOLDEN = os.path.join(REPO, "tests", "golden", "resnet_plan_parent.json")
BUF = r"(-|in|out|eps|sample|mu|logvar|ws\+\d+)"
STEP = re.compile(rf"  (\w+) u=(-?\d+) form=(\S+) set=(\d) {BUF}\+{BUF}->{BUF}\|{BUF} in=([\d,]+) out=([\d,]+) cin=(\d+) C=(\d+) s=(\d),(\d) relu=(\d) "
                  r"grid=(\d+)$")
N_CASES, N_PLANS = 5200, 330   # 15 x 2 x 33 x 5 encoder + 2 x 5 x 25 embedder cases; 240 + 90 of them are not refused


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
    exe = build(tmp_path_factory.mktemp("resnet_plan"), False)
    cases, text = run(exe)
    return {"exe": exe, "cases": cases, "text": text}


def golden(got):
    """tests/golden/resnet_plan_parent.json as {case id: {digest, lines}}.  The file keeps one `digest:lines` entry per case, grouped by
    network / configuration / batch in the order the check program prints the cases of that group; a group whose configuration repeats
    an earlier one (t3 is t8's, the bench.py pair the golden fixtures') prints the same lines and is stored as `=<that group>`."""
    groups = json.load(open(GOLDEN))["groups"]
    ids = {}
    for cid in got:
        ids.setdefault("/".join(cid.split("/")[:3]), []).append(cid)
    assert set(ids) == set(groups) and len(groups) == 40
    want = {}
    for g, entries in groups.items():
        entries = (groups[entries[1:]] if entries.startswith("=") else entries).split()
        assert len(entries) == len(ids[g]), g
        for cid, e in zip(ids[g], entries):
            want[cid] = {"digest": e.split(":")[0], "lines": int(e.split(":")[1])}
    return want


def t3(s):
    return tuple(int(v) for v in s.split(","))


def steps(case):
    out = []
    for line in case["lines"]:
        m = STEP.match(line)
        if m:
            g = m.groups()
            out.append({"kind": g[0], "unit": int(g[1]), "form": g[2], "set": int(g[3]), "src": g[4], "res": g[5], "dst": g[6], "dst16": g[7], "in": t3(g[8]),
                        "out": t3(g[9]), "cin": int(g[10]), "C": int(g[11]), "ss": int(g[12]), "st": int(g[13]), "relu": int(g[14]), "grid": int(g[15])})
        else:
            assert not line.startswith("  "), line
    return out


def refused(case):
    return case["lines"][2].startswith("refused ")


def is_down(cid, s):
    return s["kind"] == "conv" and (s["unit"] % 3 == 2 if cid.startswith("enc/") else s["unit"] > 0 and (s["unit"] - 1) % 4 == 3)


# ---------------------------------------------------------------------------------------------------------------- (a), (b), (e)

def test_every_plan_equals_the_launches_of_the_code_before_the_plans(plans):
    """Case by case against tests/golden/resnet_plan_parent.json: the fifteen encoder configurations (the eleven of encoder_cfgs.py, the
    two golden fixtures, the two of bench.py) x B 1, 3 x 1 .. 33 frames x 32, 64, 128, 256 and 64 x 128 frames, and the embedder with
    both norms x B 1, 2, 3, 5, 64 x h, w in 32, 64, 96, 128, 256.  A digest covers the workspace total, every slot offset, a refusal's
    code and text, and every launch's kind, unit, form, packed set, buffers, maps, channels, strides, ReLU and grid."""
    got = plans["cases"]
    want = golden(got)
    assert set(got) == set(want) and len(want) == N_CASES
    bad = {k: (got[k]["digest"], len(got[k]["lines"]), v) for k, v in want.items() if (got[k]["digest"], len(got[k]["lines"])) != (v["digest"], v["lines"])}
    assert not bad, dict(list(bad.items())[:5])
    assert sum(not refused(c) for c in got.values()) == N_PLANS
    # the three refusals of the encoder and the embedder's, with their codes and texts; a refused shape still has its size answered
    for cid, text in (("enc/dtdb/B1/t16/32x32", "i2v_encoder3d_forward: frame size 32x32 must be a power of two >= 64"),
                      ("enc/dtdb/B1/t11/128x128", "i2v_encoder3d_forward: 11 input frames give 6 stem frames (need a power of two)"),
                      ("enc/dtdb/B3/t16/64x64", "i2v_encoder3d_forward: the feature map is [1,2,2], conv_mu/conv_var need [1,4,4]"),
                      ("emb/bn/B2/96x64", "i2v_embedder_forward: image size 96x64 must be a power of two >= 64")):
        lines = got[cid]["lines"]
        assert lines[2] == "refused code=-1 msg=" + text and len(lines) == 3 and int(lines[0].split("=")[1]) > 0, cid
    assert not refused(got["enc/dtdb/B1/t16/128x128"]) and not refused(got["emb/in/B64/64x128"])


def test_a_perturbed_plan_is_counted(plans):
    """--perturb: the source slot of the first downsample conv of every plan that has one, else the stride of its first strided step, is
    changed before printing.  Exactly the cases with such a step miss their digest: every plan that is not refused (a residual network
    that reduces its map has a downsample branch), which is more than half of them."""
    want = golden(plans["cases"])
    got, _ = run(plans["exe"], "--perturb")
    missed = {k for k, v in want.items() if got[k]["digest"] != v["digest"]}
    n_plans = 0
    for k, c in plans["cases"].items():
        st = steps(c)
        has = any(is_down(k, s) or s["ss"] > 1 or s["st"] > 1 for s in st)
        assert (k in missed) == has, k
        n_plans += bool(st)
    assert n_plans == N_PLANS and 2 * len(missed) > n_plans


def test_sanitizer_build_prints_the_same(plans, tmp_path):
    """The check program built stand-alone with -fsanitize=address,undefined -fno-sanitize-recover=all and run directly."""
    _, text = run(build(tmp_path, True))
    assert text == plans["text"]


# ---------------------------------------------------------------------------------------------------------------- (c) slot liveness

def walk(cid, case, st):
    """One plan's steps `st` against the slot rules of test_no_step_reads_a_slot_that_is_not_live; raises AssertionError."""
    B = int(re.search(r"/B(\d+)/", cid).group(1))
    total = int(case["lines"][0].split("=")[1])
    named = {k: [int(x) for x in v.split(",")] for k, v in (f.split("=") for f in case["lines"][1].split()[1:])}
    offs = sorted({o for v in named.values() for o in v} | {total})
    room = {f"ws+{o}": offs[i + 1] - o for i, o in enumerate(offs[:-1])}
    batch_norm = case["lines"][2] == "norm=batch"
    live = {"in": None, "eps": None}   # slot -> [format, elements, [was it read]]; the two outputs of one step share the last
    assert st and st[-1]["kind"] in ("reparam", "head")
    for s in st:
        pin, pout = int(np.prod(s["in"])), int(np.prod(s["out"]))
        fmt_in = "hl16" if s["form"] in ("f16", "s2d") else "f32"
        reads = [(s["src"], fmt_in, B * (pin if s["kind"] not in ("head", "reparam") else 1) * s["cin"])]
        if s["res"] != "-":
            reads.append((s["res"], "f32", B * pout * s["C"]))
        writes = [(s[k], f, B * pout * s["C"]) for k, f in (("dst", "f32"), ("dst16", "hl16")) if s[k] != "-"]
        for slot, fmt, n in reads:
            assert slot in live, (cid, s, "reads a slot nobody wrote")
            if live[slot] is not None:
                assert live[slot][:2] == [fmt, n], (cid, s, slot, live[slot])
                live[slot][2][0] = True
        uses_stats = s["kind"] == "mean" or (s["kind"] == "norm" and not batch_norm)
        if uses_stats:
            assert B * s["C"] * 16 <= room[f"ws+{named['sums'][0]}"] and B * s["C"] * 8 <= room[f"ws+{named['coef'][0]}"], (cid, s)
        was_read = [False]
        for slot, fmt, n in writes:
            assert slot not in [r[0] for r in reads], (cid, s, "writes a slot it reads")
            if slot.startswith("ws+"):
                assert n * 4 <= room[slot], (cid, s, slot, room[slot])
                assert live.get(slot) is None or live[slot][2][0], (cid, s, slot, "overwrites a tensor nobody read")
                live[slot] = [fmt, n, was_read]
            else:
                assert slot in ("out", "sample") and s is st[-1]
        assert writes or s["kind"] == "reparam"
    assert all(v is None or v[2][0] for v in live.values()), (cid, live)


def test_no_step_reads_a_slot_that_is_not_live(plans):
    """Every plan that is not refused, step by step.  A slot is what a `ws+offset` names; its room is the distance to the next offset.
    * a step reads only what an earlier step wrote (or the caller's `in` / `eps`), in the format it takes (fp32, or the split-fp16
      operand format for the two conv16 forms) and with the element count it takes, and nothing has overwritten it since;
    * no step writes a slot it reads -- the elementwise norm kernel could run in place, but no plan uses that, so none is accepted;
    * what a step writes fits its slot, the statistics and coefficient slots included;
    * every tensor written to the workspace is read before its slot is written again or the plan ends (a write that nobody reads would
      hide a read that came too late); the fp32 and the split-fp16 output of one norm step count as one tensor, since a block reads
      its input in the one format or the other.
    The walk itself is checked on three plans made wrong by hand."""
    n = 0
    for cid, case in plans["cases"].items():
        if not refused(case):
            walk(cid, case, steps(case))
            n += 1
    assert n == N_PLANS
    cid = "enc/t8/B1/t8/64x64"
    case = plans["cases"][cid]

    def broken(edit):
        st = steps(case)
        edit(st)
        with pytest.raises(AssertionError):
            walk(cid, case, st)

    def in_place(st):       # conv2 of the first block reads the slot it writes
        next(s for s in st if s["unit"] == 1 and s["kind"] == "conv")["src"] = st[4]["dst"]

    def too_early(st):      # the downsample norm puts the residual where conv2's output waits for its norm
        next(s for s in st if s["unit"] == 3 and s["kind"] == "norm")["dst"] = st[4]["dst"]

    def wrong_format(st):   # the head reads the split-fp16 copy of the last block's output
        st[-2]["src"] = st[-3]["dst16"]

    assert steps(case)[4]["kind"] == "conv" and steps(case)[4]["unit"] == 1
    for edit in (in_place, too_early, wrong_format):
        broken(edit)


# ---------------------------------------------------------------------------------------------------------------- (d) oracles

def hooked(fn, **kw):
    """Runs fn with F.conv3d / F.conv2d recording (input shape, weight shape, stride) of every call, in order."""
    seen = []
    real = {"conv3d": F.conv3d, "conv2d": F.conv2d}

    def wrap(name):
        def f(x, w, *a, **k):
            stride = k.get("stride", 1)
            seen.append((name, tuple(x.shape), tuple(w.shape), (stride,) * (x.dim() - 2) if isinstance(stride, int) else tuple(stride)))
            return real[name](x, w, *a, **k)
        return f
    try:
        F.conv3d, F.conv2d = wrap("conv3d"), wrap("conv2d")
        with torch.no_grad():
            fn(**kw)
    finally:
        F.conv3d, F.conv2d = real["conv3d"], real["conv2d"]
    return seen


@pytest.mark.parametrize("name,frames", [("c0_16", 16), ("t8", 8)])
def test_encoder_plan_has_the_convs_of_the_oracle(plans, name, frames):
    """oracle/encoder_ref.py on one 64 x 64 clip (t8: its last layer is strided on a single frame): every F.conv3d's input map, output
    map, channels and strides are the plan's conv steps in order -- the temporal stride as it takes effect (1 on a single frame) -- and
    conv_mu / conv_var are the one head over the flattened 4 x 4 map."""
    a = ec.CASES[name]["synth"]
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in synth.encoder3d_state_dict(**a).items()}
    x = torch.zeros(1, 3, frames, 64, 64, dtype=torch.float64)
    seen = hooked(encoder_ref.encoder, sd=sd, x=x, channels=a["channels"], stride_s=a["stride_s"], stride_t=ec.CASES[name]["stride_t"])
    st = steps(plans["cases"][f"enc/{name}/B1/t{frames}/64x64"])
    convs = [s for s in st if s["kind"] in ("stem", "conv")]
    c3 = [e for e in seen if e[0] == "conv3d"]
    assert len(convs) == len(c3) and len(seen) == len(c3) + 2
    for s, (_, xs, ws, stride) in zip(convs, c3):
        out = tuple((d + 2 * (k // 2) - k) // q + 1 for d, k, q in zip(xs[2:], ws[2:], stride))
        eff = (1 if xs[2] == 1 else stride[0], stride[1])
        assert (s["in"], s["out"], s["cin"], s["C"], (s["st"], s["ss"])) == (xs[2:], out, xs[1], ws[0], eff) and stride[1] == stride[2], (s, xs, ws, stride)
    (_, xs, ws, _), (_, xs2, ws2, _) = seen[-2:]
    head = st[-2]
    assert head["kind"] == "head" and xs == xs2 and ws == ws2 and ws[2:] == xs[2:] == (4, 4)
    assert (head["cin"], head["C"]) == (xs[1] * 16, 2 * ws[0]) and st[-1]["kind"] == "reparam" and st[-1]["C"] == ws[0]
    if name == "t8":
        assert any(s["form"] == "s2d" and s["set"] == 1 and s["in"][0] == 1 for s in convs)


def test_embedder_plan_has_the_convs_of_the_oracle(plans):
    """oracle/embedder_ref.py on one 64 x 128 image: every F.conv2d in order.  The stem reads the image padded to 16 channels (the
    resize step), and fc keeps the first half of its output channels (the mean of the posterior)."""
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in synth.embedder_state_dict(seed=7, z_dim=64).items()}
    seen = hooked(embedder_ref.encode_mode, sd=sd, x=torch.zeros(1, 3, 64, 128, dtype=torch.float64))
    st = steps(plans["cases"]["emb/in/B1/64x128"])
    convs = [s for s in st if s["kind"] in ("conv", "head")]
    assert len(convs) == len(seen) == 54 and st[0]["kind"] == "resize" and (st[0]["cin"], st[0]["C"]) == (3, 16)
    for i, (s, (_, xs, ws, stride)) in enumerate(zip(convs, seen)):
        out = tuple((d + 2 * (k // 2) - k) // q + 1 for d, k, q in zip(xs[2:], ws[2:], stride))
        cin, cout = (16 if i == 0 else xs[1]), (ws[0] // 2 if s["kind"] == "head" else ws[0])
        if s["kind"] == "head":
            assert xs[2:] == (1, 1) and st[-2]["kind"] == "mean" and st[-2]["C"] == xs[1]
        assert (s["in"][1:], s["out"][1:], s["cin"], s["C"], s["ss"], s["st"]) == (xs[2:], out, cin, cout, stride[0], 1), (s, xs, ws, stride)
        assert s["form"] == ("f16" if ws[2:] == (3, 3) and stride == (1, 1) else "f32")


def test_forms_equal_encoder_paths(plans):
    """Every encoder case that is not refused: the form and packed set of conv1 of the four first blocks, and whether the block has a
    downsample conv (on the same form), are what tests/encoder_cfgs.py::encoder_paths states independently.  Where encoder_paths
    raises, the create-time rule (enc3d_halfrate_without_down, printed for all 2 x 256 stride combinations) refuses, and only there."""
    src = open(SRC).read()
    cfgs = {m.group(1): [t3(g) for g in m.groups()[1:]] for m in re.finditer(r'\{"(\w+)", \{([\d, ]+)\}, \{([\d, ]+)\}, \{([\d, ]+)\}\}', src)}
    assert len(cfgs) == 15
    for name, c in ec.CASES.items():
        assert cfgs[name] == [tuple(c["synth"]["channels"]), tuple(c["synth"]["stride_s"]), tuple(c["stride_t"])], name
    n = 0
    for cid, case in plans["cases"].items():
        if not cid.startswith("enc/") or refused(case):
            continue
        _, name, _, t, _ = cid.split("/")
        ch, ss, stt = cfgs[name]
        st = steps(case)
        got = []
        for L in range(4):
            c1 = next(s for s in st if s["kind"] == "conv" and s["unit"] == 6 * L)
            down = [s for s in st if s["kind"] == "conv" and s["unit"] == 6 * L + 2]
            assert all((d["form"], d["set"], d["src"], d["st"]) == (c1["form"], c1["set"], c1["src"], c1["st"]) for d in down)
            member = {"f16": "c1_16", "s2d": "s2d_t1" if c1["set"] else "s2d", "f32": "fp32_strided" if c1["st"] == stt[L] else "fp32_t1"}[c1["form"]]
            got.append((member, bool(down)))
        assert got == ec.encoder_paths(ch, ss, stt, int(t[1:])), cid
        n += 1
    assert n == 240
    rule = re.findall(r"^create (\w+) ss=([\d,]+) st=([\d,]+) layer=(-?\d+)$", plans["text"], re.M)
    assert len(rule) == 512
    for widths, ss, stt, layer in rule:
        ch = [64] * 5 if widths == "equal" else [32 + 16 * i for i in range(5)]
        try:
            ec.encoder_paths(ch, t3(ss), t3(stt), 16)
            raised = False
        except ValueError:
            raised = True
        assert raised == (int(layer) >= 0), (widths, ss, stt, layer)
    assert 0 < sum(int(r[3]) >= 0 for r in rule) < 256
