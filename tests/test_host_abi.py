"""CPU checks of the handle layer's contract: the ctypes table and Structure mirrors of i2v_native.py against the declarations of
include/i2v_hip.h (argument count and class, return class, struct fields), the code every handle entry answers a null handle with
(recorded from the library before the handle types shared their prologue), and the workspace carver against the alignment formula
the layout functions used to spell out one by one (tests/carver_host_check.hip, also under the host sanitizers)."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

import i2v_native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")
CSRC = os.path.join(PKG, "csrc")

SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
           "double": ctypes.c_double}
STRUCTS = {"i2v_tensor": i2v_native._Tensor, "i2v_flow_cfg": i2v_native.FlowCfg, "i2v_flow_train_layout": i2v_native.FlowTrainLayout,
           "i2v_adam_tensor": i2v_native.AdamTensor, "i2v_dec_cfg": i2v_native.DecCfg, "i2v_frames_cfg": i2v_native.FramesCfg,
           "i2v_encoder3d_cfg": i2v_native.Enc3dCfg, "i2v_vgg_layer": i2v_native.VGGLayer}
HANDLES = ("i2v_flow", "i2v_flow_train", "i2v_mlp", "i2v_gblock", "i2v_dec", "i2v_embedder", "i2v_encoder3d", "i2v_i3d", "i2v_vgg", "i2v_inception")


def _c_class(ctype):
    """'ptr', or the ctypes scalar, or None (void) of a C type as the header spells it."""
    t = re.sub(r"\bconst\b", "", ctype).strip()
    if "*" in t:
        return "ptr"
    return None if t == "void" else SCALARS[t]


def _py_class(t):
    if t is None:
        return None
    if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "ptr"
    return t


def parse_header():
    """-> ({function: (return C type, [(C type, name) per argument])}, {struct: [(field, C scalar type or 'ptr', array length or 0)]})."""
    text = open(os.path.join(REPO, "include", "i2v_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            if "*" in decl:   # one pointer per declaration
                ctype, names = "ptr", re.match(r".*\*\s*(\w+)$", decl).group(1)
            else:             # "int32_t n, t, h[2]"
                ctype, names = decl.split(None, 1)
            for n in (x.strip() for x in names.split(",")):
                arr = re.match(r"(\w+)\[(\d+)\]$", n)
                fields.append((arr.group(1) if arr else n, ctype, int(arr.group(2)) if arr else 0))
        structs[name] = fields
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = re.sub(r"typedef[^;]*;", "", text)
    text = text.replace('extern "C" {', "").replace("}", "")
    funcs = {}
    for decl in (" ".join(d.split()) for d in text.split(";") if d.strip()):
        m = re.match(r"(.*?)\b(i2v_\w+)\s*\((.*)\)$", decl)
        assert m, f"unparsed declaration: {decl[:100]}"
        args = []
        for a in (x.strip() for x in m.group(3).split(",")):
            if a and a != "void":
                am = re.match(r"(.*?)(\w+)$", a)
                args.append((am.group(1).strip(), am.group(2)))
        funcs[m.group(2)] = (m.group(1).strip(), args)
    return funcs, structs


def compare_functions(funcs, symbols):
    """Mismatches between the header's functions and a SYMBOLS-shaped table, as strings."""
    bad = [f"{n}: declared but not in the table" for n in funcs if n not in symbols] + [f"{n}: in the table but not declared" for n in symbols if n not in funcs]
    for name, (ret, args) in funcs.items():
        if name not in symbols:
            continue
        res, argtypes = symbols[name]
        if len(args) != len(argtypes):
            bad.append(f"{name}: {len(args)} arguments declared, {len(argtypes)} in the table")
            continue
        for i, ((ctype, an), t) in enumerate(zip(args, argtypes)):
            if _c_class(ctype) != _py_class(t):
                bad.append(f"{name}: argument {i} ({ctype} {an}) is {getattr(t, '__name__', t)} in the table")
        if _c_class(ret) != _py_class(res):
            bad.append(f"{name}: returns {ret}, the table says {getattr(res, '__name__', res)}")
    return bad


def compare_structs(structs):
    bad = []
    for name, fields in structs.items():
        if name not in STRUCTS:
            bad.append(f"{name}: no ctypes.Structure mirror")
            continue
        mirror = STRUCTS[name]._fields_
        if [f[0] for f in fields] != [f[0] for f in mirror]:
            bad.append(f"{name}: fields {[f[0] for f in fields]} declared, {[f[0] for f in mirror]} mirrored")
            continue
        for (fname, ctype, n), (_, t) in zip(fields, mirror):
            length = getattr(t, "_length_", 0) if isinstance(t, type) and issubclass(t, ctypes.Array) else 0
            base = t._type_ if length else t
            want = "ptr" if ctype == "ptr" else SCALARS[ctype]
            if _py_class(base) != want or length != n:
                bad.append(f"{name}.{fname}: declared {ctype}[{n}], mirrored {getattr(base, '__name__', base)}[{length}]")
    return bad + [f"{n}: mirrored but not declared" for n in STRUCTS if n not in structs]


def test_symbol_table_and_structures_match_the_header():
    """Every declaration of include/i2v_hip.h against i2v_native.SYMBOLS: argument count, per argument pointer or which of int32_t /
    int64_t / size_t / float / double, and the return class; every typedef struct against its ctypes.Structure: field names, order,
    scalar type, array length.  The comparer is shown not to be blind: an entry with an argument dropped and one with c_int32 swapped
    for c_int64 are both flagged, and so is a Structure with a field of the wrong width."""
    funcs, structs = parse_header()
    assert len(funcs) == 129 and set(funcs) == set(i2v_native.SYMBOLS)
    assert compare_functions(funcs, i2v_native.SYMBOLS) == []
    assert len(structs) == 8 and compare_structs(structs) == []

    res, args = i2v_native.SYMBOLS["i2v_dec_forward_strided"]
    assert ctypes.c_int32 in args
    dropped = dict(i2v_native.SYMBOLS, i2v_dec_forward_strided=(res, args[:-1]))
    assert compare_functions(funcs, dropped) == ["i2v_dec_forward_strided: 12 arguments declared, 11 in the table"]
    k = args.index(ctypes.c_int32)
    widened = dict(i2v_native.SYMBOLS, i2v_dec_forward_strided=(res, args[:k] + [ctypes.c_int64] + args[k + 1:]))
    flagged = compare_functions(funcs, widened)
    assert len(flagged) == 1 and flagged[0].startswith(f"i2v_dec_forward_strided: argument {k} (int32_t ")
    assert compare_functions(funcs, dict(i2v_native.SYMBOLS, i2v_flow_param_bytes=(ctypes.c_int32, [ctypes.c_void_p]))) != []

    class WrongCfg(ctypes.Structure):
        _fields_ = [(n, ctypes.c_int64 if n == "mma" else t) for n, t in i2v_native.DecCfg._fields_]
    saved, STRUCTS["i2v_dec_cfg"] = STRUCTS["i2v_dec_cfg"], WrongCfg
    try:
        assert compare_structs(structs) == ["i2v_dec_cfg.mma: declared int32_t[0], mirrored c_long[0]"]
    finally:
        STRUCTS["i2v_dec_cfg"] = saved


# The code every status-returning entry whose first parameter is a handle answers when it is called with all-zero arguments (a null
# handle), recorded from the library as it was before the handle types shared one call prologue.  -5 (I2V_E_STATE, "weights not
# loaded") at the thirteen whole-network forwards, -1 (I2V_E_INVALID) everywhere else; i2v_i3d_feature_steps returns a count: 0.
NULL_HANDLE_STATE = {"i2v_mlp_forward", "i2v_gblock_forward", "i2v_embedder_forward", "i2v_encoder3d_forward", "i2v_i3d_forward", "i2v_i3d_features",
                     "i2v_vgg_features", "i2v_vgg_features_saved", "i2v_vgg_backward", "i2v_inception_features", "i2v_dec_forward",
                     "i2v_dec_forward_strided", "i2v_dec_prepare"}
NULL_HANDLE_COUNT = {"i2v_i3d_feature_steps"}
NULL_HANDLE_INVALID = {
    "i2v_flow_load", "i2v_flow_plan", "i2v_flow_forward", "i2v_flow_inverse", "i2v_flow_train_bind", "i2v_flow_train_forward",
    "i2v_flow_train_backward", "i2v_mlp_load", "i2v_gblock_load", "i2v_gblock_status", "i2v_gblock_norm", "i2v_embedder_load",
    "i2v_encoder3d_load", "i2v_i3d_load", "i2v_i3d_unit_shape", "i2v_i3d_unit_forward", "i2v_i3d_mixed_forward", "i2v_i3d_maxpool_shape",
    "i2v_i3d_maxpool_forward", "i2v_i3d_head_forward", "i2v_vgg_load", "i2v_inception_load", "i2v_inception_block_shape",
    "i2v_inception_mixed_shape", "i2v_inception_mixed_forward", "i2v_dec_load", "i2v_dec_out_shape", "i2v_dec_prepare_cancel",
    "i2v_dec_forward_realizations", "i2v_dec_prepare_realizations", "i2v_dec_join", "i2v_dec_set_side_stream", "i2v_dec_fallback_layers",
    "i2v_dec_set_profile", "i2v_dec_debug_tap", "i2v_dec_get_spade_form", "i2v_dec_get_profile", "i2v_dec_status", "i2v_dec_get_layer_profile"}

_NULL_PROBE = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import i2v_native
lib, out = i2v_native.lib(), {}
for name in sys.argv[2:]:
    args = [None if (t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))) else
            0.0 if t in (ctypes.c_float, ctypes.c_double) else 0 for t in i2v_native.SYMBOLS[name][1]]
    rc = getattr(lib, name)(*args)
    out[name] = [int(rc), lib.i2v_last_error().decode(errors="replace")]
print("NULL_PROBE " + json.dumps(out))
"""


def test_null_handle_codes_are_the_recorded_ones():
    """One child process calls every entry of the table with all-zero arguments: it exits normally, every code is non-zero (but the
    count of i2v_i3d_feature_steps), a message is set, and each code is the recorded one."""
    funcs, _ = parse_header()
    handle = re.compile(r"(const )?(%s)\s?\*$" % "|".join(HANDLES))
    entries = [n for n, (ret, args) in funcs.items() if ret in ("int", "int32_t") and args and handle.match(args[0][0])]
    assert set(entries) == NULL_HANDLE_STATE | NULL_HANDLE_INVALID | NULL_HANDLE_COUNT and len(entries) == 13 + 39 + 1
    if not os.path.exists(i2v_native.LIB_PATH):
        pytest.skip("library not built")
    r = subprocess.run([sys.executable, "-c", _NULL_PROBE, PKG] + entries, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(re.search(r"^NULL_PROBE (.*)$", r.stdout, flags=re.M).group(1))
    want = {**{n: -5 for n in NULL_HANDLE_STATE}, **{n: -1 for n in NULL_HANDLE_INVALID}, **{n: 0 for n in NULL_HANDLE_COUNT}}
    assert {n: v[0] for n, v in got.items()} == want
    assert all(v[1] for n, v in got.items() if n not in NULL_HANDLE_COUNT), [n for n, v in got.items() if not v[1]]
    assert all(v[0] != 0 for n, v in got.items() if n not in NULL_HANDLE_COUNT)


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_carver_equals_the_written_out_alignment_rule(tmp_path, san):
    """A few thousand random slot lists (zero-sized slots, sizes around the alignment, multi-GiB slots; floats and bytes): every offset
    and the total equal o = align_up(o + bytes, 256) carried along by hand.  A stand-alone host program; with the sanitizers it is
    built with them and run directly."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path / "carver_host_check"
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if san else ["-O1"]
    r = subprocess.run([hipcc, "-std=c++17", "-Wall", "-Werror", "--offload-arch=gfx950"] + flags + ["-I" + CSRC, "-I" + os.path.join(REPO, "include"),
                        os.path.join(REPO, "tests", "carver_host_check.hip"), "-o", str(exe)], capture_output=True, text=True, timeout=900)
    if san and r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libclang_rt\.\w+san", r.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    m = re.search(r"(\d+) lists, (\d+) slots, (\d+) zero-sized, (\d+) mismatches: ok", out.stdout)
    assert m, out.stdout
    lists, slots, zeros, bad = map(int, m.groups())
    assert lists >= 2000 and slots > 10 * lists and zeros > lists and bad == 0
