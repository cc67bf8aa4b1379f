"""CPU checks of the cINN pass schedule (csrc/i2v_flow_sched.h), the one copy of the host logic that decides what happens between two
coupling half-steps.  tests/flow_sched_check.cpp, compiled for the host, prints the schedule for n_flows in {1, 2, 3, 20}, both
directions and the eight ActNorm / activation / Shuffle switch combinations; it must be (1) what the two hand-kept copies of that
logic produced before the header existed (tests/golden/flow_sched.json; its header says how it was recorded) and (2) the op order of
the reference's modules, written down here from flow_blocks.py without looking at the project's code."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")
NFS = (1, 2, 3, 20)


@pytest.fixture(scope="module")
def sched_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not (os.path.isabs(cxx) and os.path.exists(cxx)):
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("flow_sched_check") / "flow_sched_check"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(PKG, "csrc"), os.path.join(REPO, "tests", "flow_sched_check.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = {"schedules": {}, "key": None, "cond": None}
    cur = None
    for line in out.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        if kind == "schedule":
            assert rest not in got["schedules"], rest
            cur = got["schedules"].setdefault(rest, [])
        elif kind == "link":
            cur.append(rest)
        else:
            got[kind] = rest
    return got


def golden():
    return json.load(open(os.path.join(REPO, "tests", "golden", "flow_sched.json")))


def test_schedules_are_the_parents(sched_check):
    """All 64 schedules, link by link (step, Shuffle block, ActNorm block, InvLeakyRelu, swap, next half-step), equal what BOTH launch
    loops of the commit before the header computed (the golden's header states that the two agreed)."""
    g = golden()
    assert "same text" in g["parent_copies_agree"]
    want = g["schedules"]
    assert len(want) == 64 and set(sched_check["schedules"]) == set(want)
    for name, links in want.items():
        nf = int(name.split()[0].split("=")[1])
        assert len(links) == 2 * nf + 1, name
    bad = {k: (sched_check["schedules"][k], v) for k, v in want.items() if sched_check["schedules"][k] != v}
    assert not bad, bad


def _reference_ops(nf, reverse, an, act, shuf):
    """The op sequence of ConditionalFlow with n_flows = nf (flow_blocks.py:42-57: the blocks one after the other, reversed order in
    reverse), each block ConditionalFlatDoubleCouplingFlowBlock.forward (:118-136) around ConditionalDoubleVectorCouplingBlock.forward
    (:82-105).  Switched-off modules leave no op.  Reverse ops carry the suffix ^-1 (the half swap is its own inverse)."""
    ops = []
    if not reverse:
        for fl in range(nf):                                 # :44-47
            if an:
                ops.append(f"actnorm {fl}")                  # :121
            if act:
                ops.append("act")                            # :123
            for i in range(2):                               # :84
                if i % 2 != 0:
                    ops.append("swap")                       # :86-87
                ops.append(f"coupling {fl} {i}")             # :88-92
            if shuf:
                ops.append(f"shuffle {fl}")                  # :127
    else:
        for fl in reversed(range(nf)):                       # :53-56
            if shuf:
                ops.append(f"shuffle^-1 {fl}")               # :132
            for i in reversed(range(2)):                     # :98
                if i % 2 == 0:
                    ops.append("swap")                       # :99-100
                ops.append(f"coupling^-1 {fl} {i}")          # :101-104
            if act:
                ops.append("act^-1")                         # :134
            if an:
                ops.append(f"actnorm^-1 {fl}")               # :135
    return ops


def _flatten(links, reverse):
    """A schedule as an op sequence.  Inside one link the kernels apply, after the coupling, forward Shuffle, ActNorm, activation, swap
    and reverse activation^-1, ActNorm^-1, Shuffle^-1, swap (csrc/i2v_flow_sched.h, FlowLink)."""
    inv = "^-1" if reverse else ""
    ops = []
    for k, link in enumerate(links):
        f = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in link.split()}
        if k == 0:
            assert f["step"] == -1
        else:
            assert f["step"] == prepared, (k, link)    # the coupling of a link is the half-step the previous link prepared
            ops.append(f"coupling{inv} {f['step'] // 2} {f['step'] % 2}")
        prepared = f["next"]
        boundary = []
        if f["shuf"] >= 0:
            boundary.append(f"shuffle{inv} {f['shuf']}")
        if f["an"] >= 0:
            boundary.append(f"actnorm{inv} {f['an']}")
        if f["lrelu"]:
            boundary.append(f"act{inv}")
        ops += boundary[::-1] if reverse else boundary
        if f["swap"]:
            ops.append("swap")
    assert prepared == -1
    return ops


def test_schedules_are_the_references_order(sched_check):
    """Independent of the parent's code: flattened into ActNorm fl, activation, coupling (fl, i), swap, Shuffle fl, ..., every schedule
    is the reference's module order; reverse is its exact mirror with the inverse ops."""
    n = 0
    for nf in NFS:
        for rev in (False, True):
            for an in (0, 1):
                for act in (0, 1):
                    for shuf in (0, 1):
                        name = f"nf={nf} dir={'rev' if rev else 'fwd'} an={an} act={act} shuf={shuf}"
                        want = _reference_ops(nf, rev, an, act, shuf)
                        assert _flatten(sched_check["schedules"][name], rev) == want, name
                        if rev:   # the mirror property itself
                            fwd = _reference_ops(nf, False, an, act, shuf)
                            assert [o.replace("^-1", "") for o in want] == fwd[::-1], name
                        n += 1
    assert n == 64 == len(sched_check["schedules"])


def test_parameter_naming_and_cond_rule(sched_check):
    """The two loader helpers: the state_dict key of a Linear (BasicFullyConnectedNet.main holds the Linear layers at even indices,
    modules.py:14-24) and flow_blocks.py:24's rule for mode 'cond' blocks (control 0 / 1 / 2 = never / fl % 4 != 0 / always)."""
    assert sched_check["key"] == "sub_layers.0.coupling.s.0.main.0 sub_layers.19.coupling.t.1.main.6"
    want = [int(control == 2 or (control == 1 and fl % 4 != 0)) for control in range(3) for fl in range(6)]
    assert sched_check["cond"].split() == [str(v) for v in want]
