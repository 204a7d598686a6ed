"""The third ABI table (include/vstyler_clip.h, vstyler._lib.SIGNATURES_CLIP) under the rules the other
two are held to by test_abi.py, test_abi_coverage_cpu.py and test_abi_image_cpu.py: every header symbol is
exported and has a ctypes signature; the tables are disjoint; every entry maps to an existing direct test
that names it; and the entry rejects bad arguments before launching (fake aligned pointers, no device)."""
import ast
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# entry -> (file, test function, the name by which the file calls it)
COVERED = {
    "vs_clip_preprocess": ("test_clip_kernels_gpu.py", "test_clip_preprocess_exact", "vs_clip_preprocess"),
}


def header_symbols():
    src = open(os.path.join(ROOT, "include", "vstyler_clip.h")).read()
    return sorted(set(re.findall(r"^\s*(?:const char\*|int)\s+(vs_\w+)\s*\(", src, re.M)))


def test_library_exports_every_clip_header_symbol():
    from vstyler import _lib
    lib = _lib.load()
    syms = header_symbols()
    assert syms == sorted(_lib.SIGNATURES_CLIP), (syms, sorted(_lib.SIGNATURES_CLIP))
    assert not set(_lib.SIGNATURES_CLIP) & set(_lib.SIGNATURES)
    assert not set(_lib.SIGNATURES_CLIP) & set(_lib.SIGNATURES_IMAGE)
    for s in syms:
        fn = getattr(lib, s)
        assert fn.argtypes == _lib.SIGNATURES_CLIP[s], s
    assert lib.vs_abi_version() == 2
    assert len(_lib.OPTIONS) == 13           # no option ids of their own


def test_every_clip_entry_has_a_direct_test():
    from vstyler import _lib
    assert set(COVERED) == set(_lib.SIGNATURES_CLIP)
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


def test_clip_entries_reject_bad_arguments_before_launch():
    from vstyler import _lib
    lib = _lib.load()
    f = 1 << 20             # aligned, non-null, never dereferenced: validation fails first
    INVALID = 1
    # ---- vs_clip_preprocess(x, img_stride, ch_stride, row_stride, tokens, ld, n, height, width, out_size, stream)
    H, W = 48, 80
    ok = dict(x=f, ims=3 * H * W, chs=H * W, rs=W, tok=f, ld=640, n=2, h=H, w=W, size=224)
    bad = [dict(x=None), dict(tok=None), dict(n=0), dict(h=0), dict(w=-3), dict(ld=632), dict(ld=588), dict(ld=644),
           dict(tok=f + 8), dict(x=f + 1), dict(rs=W - 1), dict(chs=H * W - 1), dict(chs=-1), dict(ims=-1),
           dict(ims=3 * H * W - 1), dict(size=0), dict(size=7), dict(size=225), dict(size=910), dict(size=-14)]
    for kw in bad:
        g = dict(ok, **kw)
        rc = lib.vs_clip_preprocess(g["x"], g["ims"], g["chs"], g["rs"], g["tok"], g["ld"], g["n"], g["h"], g["w"],
                                    g["size"], None)
        assert rc == INVALID, (kw, rc)
