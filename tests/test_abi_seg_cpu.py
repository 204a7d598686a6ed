"""The fourth ABI table (include/vstyler_seg.h, vstyler._lib.SIGNATURES_SEG) under the rules the other
three are held to (test_abi.py, test_abi_coverage_cpu.py, test_abi_image_cpu.py, test_abi_clip_cpu.py): every
header symbol is exported and has a ctypes signature; the tables are disjoint; every entry maps to an
existing direct test that names it; and the entries reject bad arguments before launching (fake aligned
pointers, no device).  Also vs_epilogue.seg_rows on the entries that read it: negative under
VS_EPI_GATE_RES is VS_E_INVALID on the four GEMM entries, positive is VS_E_UNSUPPORTED on
vs_residual_layernorm."""
import ast
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID, UNSUPPORTED = 1, 3

# entry -> (file, test function, the name by which the file calls it)
COVERED = {
    "vs_layernorm_modulate_seg": ("test_seg_kernels_gpu.py", "test_layernorm_modulate_seg_equals_plain_per_slice",
                                  "layernorm_modulate_seg"),
    "vs_layernorm_modulate_fp8_seg": ("test_seg_kernels_gpu.py", "test_layernorm_modulate_seg_equals_plain_per_slice",
                                      "layernorm_modulate_fp8_seg"),
}


def header_symbols():
    src = open(os.path.join(ROOT, "include", "vstyler_seg.h")).read()
    return sorted(set(re.findall(r"^\s*(?:const char\*|int)\s+(vs_\w+)\s*\(", src, re.M)))


def test_library_exports_every_seg_header_symbol():
    from vstyler import _lib
    lib = _lib.load()
    syms = header_symbols()
    assert syms == sorted(_lib.SIGNATURES_SEG), (syms, sorted(_lib.SIGNATURES_SEG))
    for other in (_lib.SIGNATURES, _lib.SIGNATURES_IMAGE, _lib.SIGNATURES_CLIP):
        assert not set(_lib.SIGNATURES_SEG) & set(other)
    for s in syms:
        fn = getattr(lib, s)
        assert fn.argtypes == _lib.SIGNATURES_SEG[s], s
    assert lib.vs_abi_version() == 2
    assert len(_lib.OPTIONS) == 13           # no option ids of their own


def test_epilogue_struct_keeps_its_layout():
    """reserved became seg_rows: same offset, same size, and the header names it."""
    from vstyler import _lib
    f = _lib.VsEpilogue.seg_rows
    assert (f.offset, f.size) == (_lib.VsEpilogue.rows_per_batch.offset + 4, 4)
    assert ctypes.sizeof(_lib.VsEpilogue) == 72
    hdr = open(os.path.join(ROOT, "include", "vstyler.h")).read()
    body = hdr[hdr.index("typedef struct vs_epilogue"):hdr.index("} vs_epilogue;")]
    assert re.search(r"\bint seg_rows;", body) and "reserved" not in body


def test_every_seg_entry_has_a_direct_test():
    from vstyler import _lib
    assert set(COVERED) == set(_lib.SIGNATURES_SEG)
    problems = []
    for entry, (fname, test, needle) in sorted(COVERED.items()):
        path = os.path.join(HERE, fname)
        if not os.path.exists(path):
            problems.append(f"{entry}: {fname} does not exist")
            continue
        text = open(path).read()
        funcs = {n.name for n in ast.walk(ast.parse(text)) if isinstance(n, ast.FunctionDef)}
        if test not in funcs:
            problems.append(f"{entry}: {fname} has no function {test}")
        if needle not in text and entry not in text:
            problems.append(f"{entry}: {fname} names neither {needle!r} nor {entry}")
    assert not problems, "\n".join(problems)


def test_seg_entries_reject_bad_arguments_before_launch():
    from vstyler import _lib
    lib = _lib.load()
    f = 1 << 20             # aligned, non-null, never dereferenced: validation fails first
    ok = dict(x=f, ldx=3072, out=f, ldo=3072, rows=74, dim=3072, rpb=37, seg=5, shift=f, scale=f, mbs=6 * 3072,
              w=None, b=None)
    bad = [dict(x=None), dict(out=None), dict(rows=0), dict(dim=0), dict(dim=3076), dict(dim=8200), dict(ldx=3064),
           dict(ldo=3064), dict(ldx=3076), dict(x=f + 8), dict(out=f + 4), dict(shift=None), dict(scale=None),
           dict(shift=None, scale=None), dict(seg=0), dict(seg=-1), dict(shift=f + 8), dict(scale=f + 2),
           dict(mbs=6 * 3072 + 4), dict(w=f), dict(b=f), dict(w=f + 8, b=f)]
    for kw in bad:          # (out = f + 4: misaligned for the bf16 rows (16 B) and for the fp8 bytes (8 B))
        g = dict(ok, **kw)
        rc = lib.vs_layernorm_modulate_seg(g["x"], g["ldx"], g["out"], g["ldo"], g["rows"], g["dim"], g["rpb"], g["seg"],
                                           g["shift"], g["scale"], g["mbs"], g["w"], g["b"], 1e-6, None)
        assert rc == INVALID, ("bf16", kw, rc)
        rc = lib.vs_layernorm_modulate_fp8_seg(g["x"], g["ldx"], g["out"], g["ldo"], f, g["rows"], g["dim"], g["rpb"],
                                               g["seg"], g["shift"], g["scale"], g["mbs"], g["w"], g["b"], 1e-6, None)
        assert rc == INVALID, ("fp8", kw, rc)
    g = ok
    assert lib.vs_layernorm_modulate_fp8_seg(g["x"], g["ldx"], g["out"], g["ldo"], None, g["rows"], g["dim"], g["rpb"],
                                             g["seg"], g["shift"], g["scale"], g["mbs"], None, None, 1e-6,
                                             None) == INVALID


def _epi(seg_rows):
    from vstyler import _lib
    ep = _lib.VsEpilogue()
    f = 1 << 20
    ep.residual, ep.ld_res, ep.gate, ep.gate_bstride = f, 4096, f, 4096
    ep.rows_per_batch, ep.seg_rows, ep.alpha, ep.hint_scale = 1928, seg_rows, 1.0, 1.0
    return ep


def test_negative_seg_rows_is_invalid_on_every_gemm_entry():
    from vstyler import _lib
    lib = _lib.load()
    f = 1 << 20
    M, N, Kd, GATE_RES = 3856, 4096, 1024, _lib.VS_EPI_GATE_RES
    ep = _epi(-1)
    assert lib.vs_gemm(f, Kd, f, Kd, f, N, M, N, Kd, GATE_RES, ep, None, 0, None, 0, 0, None) == INVALID
    assert lib.vs_gemm_fp8(f, Kd, f, f, Kd, f, N, M, N, Kd, GATE_RES, ep, None) == INVALID
    assert lib.vs_gemm_fp8_lora(f, Kd, f, f, Kd, f, N, M, N, Kd, GATE_RES, ep, f, 64, f, 64, 64, None) == INVALID
    assert lib.vs_gemm_fp8_ws(f, Kd, f, f, Kd, f, f, N, M, N, Kd, GATE_RES, ep, None, 0, None, 0, 0, None) == INVALID
    assert lib.vs_gemm_fp8_ws(f, Kd, f, f, Kd, f, f, N, M, N, Kd, GATE_RES, ep, f, 64, f, 64, 64, None) == INVALID


def test_residual_layernorm_refuses_seg_rows():
    from vstyler import _lib
    lib = _lib.load()
    f = 1 << 20
    args = lambda ep: (f, 4096, f, 4096, f, 4096, 3856, 4096, _lib.VS_EPI_GATE_RES, ep, 0, None, None, 0, None, None,
                       1e-6, None)
    assert lib.vs_residual_layernorm(*args(_epi(5))) == UNSUPPORTED
    assert lib.vs_residual_layernorm(*args(_epi(-1))) == INVALID
