"""The fifth ABI table (include/vstyler_control.h, vstyler._lib.SIGNATURES_CONTROL) under the rules the other
four are held to (test_abi.py, test_abi_coverage_cpu.py, test_abi_image_cpu.py, test_abi_clip_cpu.py,
test_abi_seg_cpu.py): every header symbol is exported and has a ctypes signature; the tables are disjoint;
every entry maps to an existing direct test that names it; and the entries reject bad arguments before
launching (fake aligned pointers, no device)."""
import ast
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID = 1

# entry -> (file, test function, the name by which the file calls it)
COVERED = {
    "vs_ref_rows": ("test_control_kernels_gpu.py", "test_ref_rows_touches_only_the_reference_rows", "K.ref_rows("),
    "vs_unpatchify_skip": ("test_control_kernels_gpu.py", "test_unpatchify_skip", "K.unpatchify_skip("),
    "vs_camera_rays": ("test_control_kernels_gpu.py", "test_camera_rays_values", "K.camera_rays("),
    "vs_camera_im2col": ("test_control_kernels_gpu.py", "test_camera_im2col", "K.camera_im2col("),
    "vs_relu": ("test_control_kernels_gpu.py", "test_relu_every_bf16", "K.relu("),
}


def header_symbols():
    src = open(os.path.join(ROOT, "include", "vstyler_control.h")).read()
    return sorted(set(re.findall(r"^\s*(?:const char\*|int)\s+(vs_\w+)\s*\(", src, re.M)))


def test_library_exports_every_control_header_symbol():
    from vstyler import _lib
    lib = _lib.load()
    syms = header_symbols()
    assert syms == sorted(_lib.SIGNATURES_CONTROL), (syms, sorted(_lib.SIGNATURES_CONTROL))
    for other in (_lib.SIGNATURES, _lib.SIGNATURES_IMAGE, _lib.SIGNATURES_CLIP, _lib.SIGNATURES_SEG):
        assert not set(_lib.SIGNATURES_CONTROL) & set(other)
    for s in syms:
        fn = getattr(lib, s)
        assert fn.argtypes == _lib.SIGNATURES_CONTROL[s], s
    assert lib.vs_abi_version() == 2
    assert len(_lib.OPTIONS) == 13           # no option ids of their own
    assert ctypes.sizeof(_lib.VsEpilogue) == 72


def test_every_control_entry_has_a_direct_test():
    from vstyler import _lib
    assert set(COVERED) == set(_lib.SIGNATURES_CONTROL)
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


def test_control_entries_reject_bad_arguments_before_launch():
    from vstyler import _lib
    lib = _lib.load()
    f = 1 << 20             # aligned, non-null, never dereferenced: validation fails first
    _all_invalid(lib.vs_ref_rows, ("src", "bs", "dst", "ldd", "b", "n", "s", "dim"),
                 dict(src=f, bs=24 * 1536, dst=f, ldd=1536, b=2, n=24, s=72, dim=1536),
                 [dict(src=None), dict(dst=None), dict(b=0), dict(n=0), dict(s=-1), dict(dim=0), dict(dim=1532),
                  dict(ldd=1528), dict(ldd=1540), dict(src=f + 8), dict(dst=f + 2), dict(bs=24 * 1536 - 8),
                  dict(bs=24 * 1536 + 4), dict(bs=-8)])
    _all_invalid(lib.vs_unpatchify_skip, ("tok", "lat", "b", "c", "t", "h", "w", "skip"),
                 dict(tok=f, lat=f, b=2, c=16, t=3, h=8, w=12, skip=24),
                 [dict(tok=None), dict(lat=None), dict(b=0), dict(c=0), dict(t=0), dict(h=0), dict(w=0), dict(h=7),
                  dict(w=11), dict(skip=-1), dict(lat=f + 2), dict(tok=f + 1)])
    _all_invalid(lib.vs_camera_rays, ("k", "m", "out", "frames", "t", "h", "w"),
                 dict(k=f, m=f, out=f, frames=9, t=3, h=48, w=80),
                 [dict(k=None), dict(m=None), dict(out=None), dict(frames=0), dict(t=0), dict(h=0), dict(w=0),
                  dict(frames=8), dict(t=4), dict(k=f + 2), dict(m=f + 1), dict(out=f + 1)])
    _all_invalid(lib.vs_camera_im2col, ("x", "out", "ldo", "c", "t", "h", "w"),
                 dict(x=f, out=f, ldo=6144, c=24, t=3, h=64, w=96),
                 [dict(x=None), dict(out=None), dict(c=0), dict(t=0), dict(h=0), dict(w=0), dict(h=72), dict(w=88),
                  dict(ldo=6136), dict(ldo=6148), dict(x=f + 8), dict(out=f + 4)])
    _all_invalid(lib.vs_relu, ("x", "n"), dict(x=f, n=4096),
                 [dict(x=None), dict(n=0), dict(n=-8), dict(n=4100), dict(x=f + 8)])
