"""CPU-side checks of the drop-in boundary: the C-ABI libraries load without a GPU and export exactly what include/xvector_hip.h and
include/xvector_io.h declare; the two ctypes tables and the four structure mirrors match the headers type by type."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xvector_hip.h")
IO_HEADER = os.path.join(ROOT, "include", "xvector_io.h")

# C type -> (class, bytes): p pointer, i signed, u unsigned, f floating.  A type that is not listed fails the test that meets it.
C_CLASSES = {"int": ("i", 4), "int32_t": ("i", 4), "uint32_t": ("u", 4), "int64_t": ("i", 8), "uint64_t": ("u", 8),
             "long": ("i", ctypes.sizeof(ctypes.c_long)), "size_t": ("u", ctypes.sizeof(ctypes.c_size_t)),
             "uintptr_t": ("u", ctypes.sizeof(ctypes.c_void_p)), "float": ("f", 4), "double": ("f", 8), "void": None}
POINTER = ("p", ctypes.sizeof(ctypes.c_void_p))
STRUCT = r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;"


def _code(path):
    """(the header without comments and preprocessor lines, its integer #defines)."""
    src = open(path).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(\w+)\s+(\d+)\b", src, flags=re.M)}
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#")), defines


def _c_class(decl, defines):
    """(class, bytes[, array length]) of a C declaration `type [name]`, `type* [name]` or `type name[N]`."""
    decl = " ".join(decl.replace("*", " * ").split())
    array = re.search(r"\[\s*(\w*)\s*\]$", decl)
    if array:
        decl = decl[:array.start()].strip()
    words = [w for w in decl.split() if w != "const"]
    if "*" in words:
        assert not array, decl
        return POINTER
    assert 1 <= len(words) <= 2 and words[0] in C_CLASSES, "a C type this test does not know: `%s`" % decl
    if array:
        assert len(words) == 2, decl
        n = array.group(1)
        return C_CLASSES[words[0]] + (defines[n] if n in defines else int(n),)
    return C_CLASSES[words[0]]


def _ctypes_class(t):
    if t is None:
        return None
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return POINTER
    if issubclass(t, ctypes.Array):
        return _ctypes_class(t._type_) + (t._length_,)
    assert issubclass(t, ctypes._SimpleCData) and t._type_ in "bhilqBHILQfd", "a ctypes type this test does not know: %r" % (t,)
    return ("f" if t._type_ in "fd" else "i" if t._type_ in "bhilq" else "u", ctypes.sizeof(t))


def header_prototypes(path):
    """[(name, return class, [parameter classes])] of every prototype."""
    src, defines = _code(path)
    src = re.sub(STRUCT, "", src, flags=re.S)
    out = []
    for ret, name, params in re.findall(r"([^;{}()]*?)\b(xv(?:io)?_\w+)\s*\(([^()]*)\)\s*;", src):
        params = [] if params.strip() in ("", "void") else params.split(",")
        # (`T name[N]` as a parameter is a pointer)
        out.append((name, _c_class(ret, defines), [POINTER if p.strip().endswith("]") else _c_class(_unnamed(p), defines) for p in params]))
    assert src.count(");") == len(out), "%s: %d statements end in `);`, %d were read as prototypes" % (path, src.count(");"), len(out))
    return out


def _unnamed(param):
    """`const float* x` -> `const float*`: the parameter's name is dropped (every parameter in the headers has one)."""
    m = re.match(r"^(.*[\s*])(\w+)\s*$", param.strip(), flags=re.S)
    assert m, "a parameter without a name or a type: `%s`" % param
    return m.group(1)


def header_struct(path, name):
    """[(field, class)] of `typedef struct name { ... } name;` in declaration order."""
    src, defines = _code(path)
    body = [m.group(2) for m in re.finditer(STRUCT, src, flags=re.S) if m.group(1) == name]
    assert len(body) == 1, (path, name)
    fields = []
    for decl in body[0].split(";"):
        if not decl.strip():
            continue
        first, *more = decl.split(",")                           # `int32_t min_len, max_len`: the type belongs to every name
        base = re.match(r"^(.*[\s*])(\w+(\[\w*\])?)\s*$", first.strip(), flags=re.S)
        assert base, decl
        for field in [base.group(2)] + [m.strip() for m in more]:
            fields.append((field.split("[")[0], _c_class(base.group(1) + " " + field, defines)))
    return fields


def check_signatures(path, table):
    protos = header_prototypes(path)
    assert sorted(p[0] for p in protos) == sorted(table) and len(protos) == len(table), "the table and the header list different names"
    for name, ret, params in protos:
        res, args = table[name]
        assert _ctypes_class(res) == ret, "%s: returns %r in the header, %r in the table" % (name, ret, _ctypes_class(res))
        for i, (a, c) in enumerate(zip(args, params)):
            assert _ctypes_class(a) == c, "%s: parameter %d is %r in the header, %r in the table" % (name, i, c, _ctypes_class(a))
        assert len(args) == len(params), "%s: %d parameters in the header, %d in the table" % (name, len(params), len(args))


def check_struct(path, name, mirror):
    assert [(n, _ctypes_class(t)) for n, t in mirror._fields_] == header_struct(path, name)


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(xv_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_header_declares_entry_points():
    names = header_functions()
    assert len(names) >= 40
    for must in ("xv_affine_forward", "xv_affine_dgrad", "xv_affine_wgrad", "xv_stat_pool_forward",
                 "xv_margin_softmax_rows", "xv_engine_create", "xv_engine_forward", "xv_engine_backward"):
        assert must in names


def test_library_loads_and_exports_every_symbol():
    from tf_kaldi_speaker_amd import _lib
    assert os.path.isfile(_lib.LIB_PATH), "build the HIP extension first (__graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in header_functions():
        assert hasattr(lib, name), "libxvector_hip.so does not export %s" % name


def test_ctypes_table_matches_header():
    from tf_kaldi_speaker_amd import _lib
    assert sorted(_lib.SIGNATURES) == header_functions()
    lib = _lib.load()
    assert lib.xv_abi_version() == _lib.ABI_VERSION
    assert lib.xv_device_count() >= 0   # 0 here: no compute call is made without a GPU


def test_signature_tables_match_the_prototypes_type_by_type():
    """Return type and every parameter of all prototypes of both headers against the two SIGNATURES tables, by C class (pointer, signed /
    unsigned integer and floating type of a size): a c_int where the header says size_t, or a missing pointer, corrupts a call on the GPU
    and is invisible to a comparison of names."""
    from tf_kaldi_speaker_amd import _lib
    from tf_kaldi_speaker_amd.dataset import native_loader
    assert len(header_prototypes(HEADER)) == len(_lib.SIGNATURES) >= 118
    check_signatures(HEADER, _lib.SIGNATURES)
    check_signatures(IO_HEADER, native_loader.SIGNATURES)
    with pytest.raises(AssertionError, match="does not know"):
        _c_class("hipStream_t stream", {})
    with pytest.raises(AssertionError, match="does not know"):
        _ctypes_class(ctypes.c_longdouble)
    assert _c_class("const float** x", {}) == _c_class("const char*", {}) == POINTER
    assert _c_class("int32_t shape[N]", {"N": 4}) == ("i", 4, 4) and _c_class("const uint64_t", {}) == ("u", 8)


def test_struct_layouts_match_headers():
    """Field order, field type and array length of the four structures that cross the boundary == their ctypes mirrors."""
    from tf_kaldi_speaker_amd import _lib
    from tf_kaldi_speaker_amd.dataset import native_loader
    check_struct(HEADER, "xv_config", _lib.XvConfig)
    check_struct(HEADER, "xv_mfcc_config", _lib.XvMfccConfig)
    check_struct(HEADER, "xv_augment_config", _lib.XvAugmentConfig)
    check_struct(IO_HEADER, "xvio_config", native_loader.XvioConfig)
    fields = dict(header_struct(HEADER, "xv_config"))
    assert fields["frame_context"] == ("i", 4, 12) and fields["margin_m"] == ("f", 4) and len(fields) == len(_lib.XvConfig._fields_)
    assert dict(header_struct(IO_HEADER, "xvio_config"))["data_dir"] == POINTER
    assert _lib.XV_MAX_FRAME_LAYERS == 12 and "#define XV_MAX_FRAME_LAYERS 12" in open(HEADER).read()


def test_config_mirrors_take_keywords_only_and_fill_in_struct_bytes():
    from tf_kaldi_speaker_amd import _lib
    for cls in (_lib.XvConfig, _lib.XvMfccConfig, _lib.XvAugmentConfig):
        with pytest.raises(TypeError, match="^%s takes keyword arguments only \\(its first field is struct_bytes, filled in here\\)$" % cls.__name__):
            cls(30)
        assert cls().struct_bytes == ctypes.sizeof(cls) and cls(struct_bytes=1).struct_bytes == ctypes.sizeof(cls)
    assert _lib.XvConfig.DEFAULTS == {} and _lib.XvConfig().feat_dim == 0 and _lib.XvConfig(feat_dim=30).feat_dim == 30
    m = _lib.XvMfccConfig(num_ceps=24)
    assert (m.num_ceps, m.num_mel_bins, m.sample_frequency) == (24, 30, 16000.0)
    a = _lib.XvAugmentConfig(volume=0.5)
    assert (a.volume, a.shift_output, a.normalize_output) == (0.5, 1, 1)


def test_engine_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from tf_kaldi_speaker_amd import engine
    with pytest.raises(engine.XvError):
        engine.Engine(engine.make_config(30, 10))


def test_environment_switches_are_value_checked_and_unknown_ones_named():
    """the library reads a few documented switches; a value it does not understand makes engine creation fail with
    the name - before any GPU call, so this runs here.  Any other XV_* variable (a typo, a switch of an earlier round, another program's) is
    named once on stderr and ignored: it must not stop a run."""
    import subprocess
    import sys
    code = ("import ctypes as C, sys; sys.path.insert(0, %r)\n"
            "from tf_kaldi_speaker_amd import _lib\n"
            "lib = _lib.load(); cfg = _lib.XvConfig(); cfg.feat_dim = 30; h = C.c_void_p()\n"
            "rc = lib.xv_engine_create(C.byref(cfg), C.byref(h)); print(rc, lib.xv_last_error().decode())\n" % ROOT)
    for extra, want in (({"XV_NT_SCHED": "fast"}, "XV_NT_SCHED=fast: expected dp or sk"), ({"XV_CONV_WR": "3"}, "XV_CONV_WR=3: expected 2 or 4"),
                        ({"XV_SEGMENT_FUSED": "yes"}, "XV_SEGMENT_FUSED=yes: expected 0 or 1")):
        env = {k: v for k, v in os.environ.items() if not k.startswith("XV_")}
        env.update(extra)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.startswith("2 ") and want in out.stdout, (out.stdout, out.stderr[-500:])
    env = {k: v for k, v in os.environ.items() if not k.startswith("XV_")}
    env.update(XV_NT_SCHED="dp", XV_PRECISION="f32", XV_SHARE_GPU="1")          # documented names pass the table (the call then fails later: no GPU here)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert "environment switch" not in out.stdout + out.stderr and "expected" not in out.stdout, (out.stdout, out.stderr[-500:])
    env.update(XV_TN_WGS="768")                                                 # not a name of this package: named on stderr, not a failure
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert "ignoring unknown environment switch XV_TN_WGS" in out.stderr and "environment switch" not in out.stdout, (out.stdout, out.stderr[-500:])


def test_config_struct_size_is_checked():
    """xv_config.struct_bytes (ABI version 2): a host built against another header's xv_config is refused at xv_engine_create instead of
    having fields read from beyond its struct."""
    import ctypes as C
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    assert lib.xv_abi_version() == _lib.ABI_VERSION == 3
    cfg = _lib.XvConfig()
    assert cfg.struct_bytes == C.sizeof(_lib.XvConfig)
    cfg.feat_dim = 30
    cfg.struct_bytes -= 4
    h = C.c_void_p()
    assert lib.xv_engine_create(C.byref(cfg), C.byref(h)) != 0
    assert "struct_bytes" in lib.xv_last_error().decode()
