"""The sixth ABI table (include/vstyler_vae22.h, vstyler._lib.SIGNATURES_VAE22) under the rules the other
five are held to (test_abi.py, test_abi_coverage_cpu.py, test_abi_image_cpu.py, test_abi_clip_cpu.py,
test_abi_seg_cpu.py, test_abi_control_cpu.py): every header symbol is exported and has a ctypes signature;
the tables are disjoint; every entry maps to an existing direct test that names it; and the entries reject
bad arguments before launching (fake aligned pointers, no device)."""
import ast
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID = 1

# entry -> (file, test function, the name by which the file calls it)
COVERED = {
    "vs_vae22_rmsnorm": ("test_vae22_kernels_gpu.py", "test_wide_rmsnorm", "vs_vae22_rmsnorm("),
    "vs_vae22_avgdown_add": ("test_vae22_kernels_gpu.py", "test_avgdown_exact_sums", "vae.avgdown_add("),
    "vs_vae22_dupup_add": ("test_vae22_kernels_gpu.py", "test_dupup_bit_exact", "vae.dupup_add("),
    "vs_vae22_patchify": ("test_vae22_kernels_gpu.py", "test_patchify_bit_exact", "vs_vae22_patchify("),
    "vs_vae22_unpatchify": ("test_vae22_kernels_gpu.py", "test_unpatchify_bit_exact", "vs_vae22_unpatchify("),
    "vs_vae22_softmax_split": ("test_vae22_kernels_gpu.py", "test_softmax_split", "vs_vae22_softmax_split("),
}


def header_symbols():
    src = open(os.path.join(ROOT, "include", "vstyler_vae22.h")).read()
    return sorted(set(re.findall(r"^\s*(?:const char\*|int)\s+(vs_\w+)\s*\(", src, re.M)))


def test_library_exports_every_vae22_header_symbol():
    from vstyler import _lib
    lib = _lib.load()
    syms = header_symbols()
    assert syms == sorted(_lib.SIGNATURES_VAE22), (syms, sorted(_lib.SIGNATURES_VAE22))
    for other in (_lib.SIGNATURES, _lib.SIGNATURES_IMAGE, _lib.SIGNATURES_CLIP, _lib.SIGNATURES_SEG,
                  _lib.SIGNATURES_CONTROL):
        assert not set(_lib.SIGNATURES_VAE22) & set(other)
    for s in syms:
        fn = getattr(lib, s)
        assert fn.argtypes == _lib.SIGNATURES_VAE22[s], s
    assert lib.vs_abi_version() == 2
    assert len(_lib.OPTIONS) == 13           # no option ids of their own
    assert ctypes.sizeof(_lib.VsEpilogue) == 72


def test_every_vae22_entry_has_a_direct_test():
    from vstyler import _lib
    assert set(COVERED) == set(_lib.SIGNATURES_VAE22)
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


def _all_invalid(fn, order, ok, bad):
    for kw in bad:
        g = dict(ok, **kw)
        rc = fn(*[g[k] for k in order], None)
        assert rc == INVALID, (fn.__name__, kw, rc)


def test_vae22_entries_reject_bad_arguments_before_launch():
    from vstyler import _lib
    lib = _lib.load()
    f = 1 << 20             # aligned, non-null, never dereferenced: validation fails first
    _all_invalid(lib.vs_vae22_rmsnorm, ("x", "ldx", "y", "ldy", "g", "npix", "c", "silu"),
                 dict(x=f, ldx=1024, y=f, ldy=1024, g=f, npix=70, c=1024, silu=1),
                 [dict(x=None), dict(y=None), dict(g=None), dict(c=0), dict(c=1056, ldx=1056, ldy=1056),
                  dict(c=40, ldx=40, ldy=40), dict(ldx=1016), dict(ldy=1016), dict(ldx=1028), dict(ldy=1028),
                  dict(npix=-1), dict(x=f + 8), dict(y=f + 8), dict(g=f + 8)])
    shortcut = ("x", "y", "n", "t", "h", "w", "ci", "co", "ft", "fs")
    _all_invalid(lib.vs_vae22_avgdown_add, shortcut,
                 dict(x=f, y=f, n=2, t=5, h=4, w=6, ci=160, co=320, ft=2, fs=2),
                 [dict(x=None), dict(y=None), dict(n=0), dict(t=0), dict(h=0), dict(w=0), dict(ci=0), dict(co=0),
                  dict(t=4), dict(co=336), dict(ci=164), dict(co=324), dict(ft=3), dict(fs=0), dict(fs=3), dict(h=5),
                  dict(w=7), dict(x=f + 8), dict(y=f + 2)])
    _all_invalid(lib.vs_vae22_dupup_add, shortcut,
                 dict(x=f, y=f, n=2, t=3, h=2, w=3, ci=1024, co=512, ft=2, fs=2),
                 [dict(x=None), dict(y=None), dict(n=0), dict(t=0), dict(h=0), dict(w=0), dict(ci=0), dict(co=0),
                  dict(ci=1032), dict(co=516), dict(ci=1028), dict(ft=0), dict(ft=3), dict(fs=4), dict(x=f + 8),
                  dict(y=f + 4)])
    _all_invalid(lib.vs_vae22_patchify, ("src", "ld", "dst", "nt", "h", "w"),
                 dict(src=f, ld=4, dst=f, nt=5, h=6, w=10),
                 [dict(src=None), dict(dst=None), dict(nt=0), dict(h=0), dict(w=0), dict(h=7), dict(w=9), dict(ld=3),
                  dict(ld=6), dict(ld=0), dict(src=f + 4), dict(dst=f + 8)])
    # the inverse has no parity rule (its h, w are the patch grid's); its row must hold the 12 channels
    _all_invalid(lib.vs_vae22_unpatchify, ("src", "ld", "dst", "nt", "h", "w"),
                 dict(src=f, ld=16, dst=f, nt=5, h=3, w=5),
                 [dict(src=None), dict(dst=None), dict(nt=0), dict(h=0), dict(w=0), dict(ld=8), dict(ld=14),
                  dict(src=f + 4), dict(dst=f + 8)])
    _all_invalid(lib.vs_vae22_softmax_split, ("s", "ld_s", "p", "ld_p", "rows", "ncols"),
                 dict(s=f, ld_s=32, p=f, ld_p=64, rows=10, ncols=24),
                 [dict(s=None), dict(p=None), dict(ncols=0), dict(ld_s=23), dict(ld_p=63), dict(ld_p=46), dict(rows=-1),
                  dict(s=f + 2), dict(p=f + 1)])
