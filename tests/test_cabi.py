"""The C-ABI library loads without a GPU and exports exactly what include/b4r.h declares; host-only queries (layouts,
argument validation, error messages) work on CPU.  No compute call is made here."""
import ctypes as C
import os
import re

import pytest

from bert4rec_amd import _lib
from bert4rec_amd.engine import make_model_config, param_table
from oracle import bert4rec_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, "include", "b4r.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(b4r_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    syms = header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/b4r.h but not exported"
    assert sorted(_lib.PROTOTYPES) == syms, "bert4rec_amd/_lib.py PROTOTYPES and include/b4r.h disagree"
    assert lib.b4r_version() == 100


def test_struct_sizes_match_the_header():
    assert C.sizeof(_lib.ModelConfig) == 36 and C.sizeof(_lib.AdamWConfig) == 48   # 9 x 4 bytes, padding, the decay-mask pointer
    assert C.sizeof(_lib.Batch) == 4 * 8 + 3 * 4 + 4     # padded to 8
    assert _lib.STATE_WORDS * 4 == 64


def strip_c_comments(text):
    """comments out, line numbers kept"""
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


# ---- include/b4r.h against bert4rec_amd/_lib.py: every argument list, return type and structure field ------------------------------
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32,
           "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
MIRRORS = {"b4r_model_config": _lib.ModelConfig, "b4r_model_config_ex": _lib.ModelConfigEx, "b4r_batch": _lib.Batch,
           "b4r_adamw_config": _lib.AdamWConfig, "b4r_item_quota": _lib.ItemQuota, "b4r_gemm_desc": _lib.GemmDesc,
           "b4r_gemm_tn_desc": _lib.GemmTnDesc, "b4r_attn_block_desc": _lib.AttnBlockDesc,
           "b4r_attn_block_bwd_desc": _lib.AttnBlockBwdDesc, "b4r_ffn_desc": _lib.FfnDesc}


def ctypes_allowed(ctype):
    """the ctypes types that may stand for the C type `ctype` (a return type, a parameter's type or a field's)"""
    t = " ".join(w for w in ctype.replace("*", " * ").split() if w != "const")
    if t == "b4r_stream_t" or t == "void *":
        return [C.c_void_p]
    if t == "char *":
        return [C.c_char_p]
    if t.endswith(" *"):
        base = t[:-2]
        if base in MIRRORS:
            return [C.POINTER(MIRRORS[base])]
        return [C.c_void_p] + ([C.POINTER(SCALARS[base])] if base in SCALARS else [])   # b4r_train_state*: opaque
    return [MIRRORS[t] if t in MIRRORS else SCALARS[t]]    # KeyError: a type this parse does not know


def parse_header():
    text = strip_c_comments(open(os.path.join(ROOT, "include", "b4r.h")).read())
    consts = {k: int(v) for k, v in re.findall(r"\b(B4R_\w+) = (-?\d+)", text)}
    structs = {}
    for body, name in re.findall(r"typedef struct \w+ \{(.*?)\}\s*(\w+);", text, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            ctype, names = re.fullmatch(r"(.*?[\s*])(\w+(?:\[\w+\])?(?:\s*,\s*\w+(?:\[\w+\])?)*)", decl, flags=re.S).groups()
            for n in re.split(r"\s*,\s*", names):
                n, dim = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", n).groups()
                fields.append((n, ctype, None if dim is None else consts[dim] if dim in consts else int(dim)))
        structs[name] = fields
    protos = {}
    for ret, name, args in re.findall(r"^([\w ]+?[\s*]+)(b4r_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        args = [] if args.strip() == "void" else [re.fullmatch(r"(.*?[\s*])\w+", a.strip(), flags=re.S).group(1) for a in args.split(",")]
        protos[name] = (ret, args)
    return structs, protos


def test_lib_py_mirrors_the_header():
    structs, protos = parse_header()
    wrong = []
    assert set(MIRRORS) <= set(structs)
    for cname, cls in MIRRORS.items():
        want = [(n, ctype, dim) for n, ctype, dim in structs[cname]]
        if [n for n, _, _ in want] != [f[0] for f in cls._fields_]:
            wrong.append(f"{cname}: field names {[n for n, _, _ in want]} != {[f[0] for f in cls._fields_]}")
            continue
        for (n, ctype, dim), (_, got) in zip(want, cls._fields_):
            if dim is not None:
                ok = issubclass(got, C.Array) and got._length_ == dim and got._type_ in ctypes_allowed(ctype)
            else:
                ok = got in ctypes_allowed(ctype)
            if not ok:
                wrong.append(f"{cname}.{n}: {ctype.strip()}{'' if dim is None else [dim]} mirrored as {got.__name__}")
    assert sorted(protos) == sorted(_lib.PROTOTYPES)
    for name, (ret, args) in protos.items():
        restype, argtypes = _lib.PROTOTYPES[name]
        if restype not in ctypes_allowed(ret):
            wrong.append(f"{name}: returns {ret.strip()}, mirrored as {restype.__name__}")
        if len(args) != len(argtypes):
            wrong.append(f"{name}: {len(args)} arguments, mirrored with {len(argtypes)}")
            continue
        for i, (a, got) in enumerate(zip(args, argtypes)):
            if got not in ctypes_allowed(a):
                wrong.append(f"{name}: argument {i} is {a.strip()}, mirrored as {got.__name__}")
    assert not wrong, "bert4rec_amd/_lib.py does not mirror include/b4r.h:\n" + "\n".join(wrong)
    assert len(protos) >= 123 and all(len(structs[c]) == len(MIRRORS[c]._fields_) for c in MIRRORS)


# ---- the library's own translation units: b4r_ prototypes stand in headers only ----------------------------------
ARGS = r"\((?:[^()]|\([^()]*\))*\)"
DECL = r'^(?:extern "C" )?((?:[\w:<>]+[ \t*&]+)+)(b4r_\w+)\s*' + ARGS + r"\s*"


def test_internal_launchers_are_declared_in_headers_only():
    csrc = os.path.join(ROOT, "bert4rec_amd", "csrc")
    text = {n: strip_c_comments(open(os.path.join(csrc, n)).read()) for n in sorted(os.listdir(csrc)) if n.endswith((".hip", ".h"))}
    hips = {n: t for n, t in text.items() if n.endswith(".hip")}
    copies = [f"{n}:{t.count(chr(10), 0, m.start()) + 1}" for n, t in hips.items() for m in re.finditer(DECL + ";", t, flags=re.M)]
    assert not copies, "b4r_ prototypes outside the headers: " + ", ".join(copies)
    declared = [m.group(2) for h in ("b4r_internal.h", "b4r_common.h") for m in re.finditer(DECL + ";", text[h], flags=re.M)]
    assert len(declared) >= 60 and len(set(declared)) == len(declared), "a function is declared twice"
    defined = [(m.group(2), n, m.group(1)) for n, t in hips.items() for m in re.finditer(DECL + r"\{", t, flags=re.M)]
    for fn in declared:
        where = [(n, quals) for f, n, quals in defined if f == fn]
        assert len(where) == 1 and "static" not in where[0][1].split(), f"{fn}: declared in a header, defined in {where}"


def test_parameter_layout_ml1m():
    lib = _lib.load()
    cfg = make_model_config(3709, 64, 2, 2, 200, 256, 0.2, 0.2)
    table = param_table(cfg)
    assert sum(e.rows * e.cols for e in table) == 358269           # trainable floats at C1
    assert lib.b4r_param_total_floats(C.byref(cfg)) == 358272      # + padding of the [3709] output bias
    n_decay = lib.b4r_param_decay_floats(C.byref(cfg))
    # names and shapes are the reference's Keras variables; decay flags follow adam_w_optimizer.py:154-168
    ocfg = orc.OracleConfig(vocab_size=3709)
    want = {n: s for n, s in orc.param_names_and_shapes(ocfg) if orc.is_trainable(n)}
    assert {e.name for e in table} == set(want)
    for e in table:
        size = 1
        for d in want[e.name]:
            size *= d
        assert e.rows * e.cols == size, e.name
        assert bool(e.decay) == orc.uses_weight_decay(e.name), e.name
        assert (e.offset < n_decay) == bool(e.decay), e.name
        assert e.offset % 4 == 0
    q = next(e for e in table if e.name.endswith("layer_1/self_attention/key/kernel"))
    assert (q.rows, q.cols, q.ld) == (64, 64, 192)                  # column block of the fused [H,3H] QKV matrix
    assert lib.b4r_pooler_floats(C.byref(cfg)) == 64 * 64 + 64


def test_workspace_queries_and_regions():
    lib = _lib.load()
    cfg = make_model_config(3709, 64, 2, 2, 200, 256)
    nbytes = lib.b4r_workspace_bytes(C.byref(cfg), 256, 200, 40)
    assert nbytes > 256 * 40 * 3709 * 4
    off, rows, cols, ld = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.b4r_workspace_region(C.byref(cfg), 256, 200, 40, b"mlm_logits", C.byref(off), C.byref(rows), C.byref(cols), C.byref(ld)) == 0
    assert (rows.value, cols.value, ld.value) == (10240, 3709, 3712) and off.value % 4 == 0
    assert lib.b4r_workspace_region(C.byref(cfg), 256, 200, 40, b"encoder_output_1", C.byref(off), C.byref(rows), C.byref(cols), C.byref(ld)) == 0
    assert (rows.value, cols.value) == (51200, 64)
    assert lib.b4r_workspace_region(C.byref(cfg), 256, 200, 40, b"nonsense", C.byref(off), C.byref(rows), C.byref(cols), C.byref(ld)) == -1
    assert "unknown region" in _lib.last_error()


@pytest.mark.parametrize("bad", [dict(hidden=96, heads=3), dict(hidden=64, heads=4), dict(hidden=2048, heads=64), dict(layers=0)])
def test_invalid_geometry_is_reported_not_crashed(bad):
    lib = _lib.load()
    cfg = make_model_config(100, bad.get("hidden", 64), bad.get("layers", 2), bad.get("heads", 2), 50, 256)
    assert lib.b4r_param_total_floats(C.byref(cfg)) == -1
    assert len(_lib.last_error()) > 0


def test_null_arguments_return_error_codes():
    lib = _lib.load()
    assert lib.b4r_gemm_f32(None, None) == -1 and "null" in _lib.last_error()
    assert lib.b4r_state_begin_step(None, None) == -1
    d = _lib.GemmDesc()
    d.A = d.B = d.C = 16
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = 4, 4, 8, 4, 4, 4     # lda < K
    assert lib.b4r_gemm_f32(C.byref(d), None) == -2


def test_native_library_reads_no_environment():
    # a switch read from the environment is fixed for the life of a process, so the suite could only ever run its default: every
    # path of the library must follow from shapes, modes, flags and ABI setters, which the tests vary
    csrc = os.path.join(ROOT, "bert4rec_amd", "csrc")
    readers = []
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h", ".cpp", ".cc", ".c")):
            text = open(os.path.join(csrc, name)).read()
            readers += [f"{name}:{text.count(chr(10), 0, m.start()) + 1}" for m in re.finditer(r"\b(secure_)?getenv\s*\(", text)]
    assert not readers, "environment reads in the native library: " + ", ".join(readers)
