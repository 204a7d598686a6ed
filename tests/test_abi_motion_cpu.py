"""The eighth ABI table (include/vstyler_motion.h, vstyler._lib.SIGNATURES_MOTION) under the rules the other
tables are held to (test_abi.py, test_abi_coverage_cpu.py, test_abi_animate_cpu.py, ...): every header symbol is
exported and has a ctypes signature; the tables are disjoint; every entry maps to an existing direct test that
names it; and the entries reject bad arguments before launching (fake aligned pointers, no device)."""
import ast
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID = 1

# entry -> (file, test function, the name by which the file calls it)
COVERED = {
    "vs_motion_stem": ("test_motion_kernels_gpu.py", "test_stem_every_byte", "K.motion_stem("),
    "vs_lrelu_blur": ("test_motion_kernels_gpu.py", "test_blur_exact", "K.lrelu_blur("),
    "vs_lrelu_merge": ("test_motion_kernels_gpu.py", "test_act_every_bf16", "K.lrelu_merge("),
    "vs_motion_direction": ("test_motion_kernels_gpu.py", "test_direction", "K.motion_direction("),
}


def header_symbols():
    src = open(os.path.join(ROOT, "include", "vstyler_motion.h")).read()
    return sorted(set(re.findall(r"^\s*(?:const char\*|int)\s+(vs_\w+)\s*\(", src, re.M)))


def test_library_exports_every_motion_header_symbol():
    from vstyler import _lib
    lib = _lib.load()
    syms = header_symbols()
    assert syms == sorted(_lib.SIGNATURES_MOTION), (syms, sorted(_lib.SIGNATURES_MOTION))
    for other in (_lib.SIGNATURES, _lib.SIGNATURES_IMAGE, _lib.SIGNATURES_CLIP, _lib.SIGNATURES_SEG,
                  _lib.SIGNATURES_CONTROL, _lib.SIGNATURES_VAE22, _lib.SIGNATURES_ANIMATE):
        assert not set(_lib.SIGNATURES_MOTION) & set(other)
    for s in syms:
        fn = getattr(lib, s)
        assert fn.argtypes == _lib.SIGNATURES_MOTION[s], s
    assert lib.vs_abi_version() == 2
    assert len(_lib.OPTIONS) == 13           # no option ids of their own
    assert ctypes.sizeof(_lib.VsEpilogue) == 72
    assert ctypes.sizeof(_lib.VsConv3d) == 224      # vs_conv3d keeps its size


def test_every_motion_entry_has_a_direct_test():
    from vstyler import _lib
    assert set(COVERED) == set(_lib.SIGNATURES_MOTION)
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


def _all(fn, order, ok, bad):
    for kw in bad:
        g = dict(ok, **kw)
        rc = fn(*[g[k] for k in order], None)
        assert rc == INVALID, (fn.__name__, kw, rc)


def test_motion_entries_reject_bad_arguments_before_launch():
    from vstyler import _lib
    lib = _lib.load()
    f = 1 << 20             # aligned, non-null, never dereferenced: validation fails first
    far = 1 << 30           # a second buffer that overlaps nothing
    w, b = 1 << 28, (1 << 28) + 4096
    # the stem: 2 frames of 8 x 8, 32 channels in rows of 40
    order = ("x", "u8", "wt", "bias", "y", "yns", "ldy", "n", "h", "w", "c0")
    ok = dict(x=f, u8=1, wt=w, bias=b, y=far, yns=64 * 40, ldy=40, n=2, h=8, w=8, c0=32)
    _all(lib.vs_motion_stem, order, ok,
         [dict(x=None), dict(wt=None), dict(bias=None), dict(y=None), dict(n=0), dict(h=0), dict(w=0), dict(c0=0),
          dict(c0=28), dict(c0=520), dict(ldy=24), dict(ldy=36), dict(yns=63 * 40 + 24), dict(yns=64 * 40 + 4),
          dict(wt=w + 8), dict(bias=b + 8), dict(y=far + 8), dict(u8=0, x=f + 1),
          dict(y=f), dict(y=f + 16), dict(y=w), dict(y=b)])
    # the blur: 2 frames of 5 x 7, 40 channels in rows of 48, pad (2, 2) step 1 -> 6 x 8
    order = ("x", "xns", "ldx", "y", "yns", "ldy", "bias", "n", "h", "w", "c", "p0", "p1", "step")
    ok = dict(x=f, xns=35 * 48, ldx=48, y=far, yns=48 * 48, ldy=48, bias=b, n=2, h=5, w=7, c=40, p0=2, p1=2, step=1)
    _all(lib.vs_lrelu_blur, order, ok,
         [dict(x=None), dict(y=None), dict(n=0), dict(h=0), dict(w=0), dict(c=0), dict(c=36), dict(p0=-1), dict(p0=4),
          dict(p1=-1), dict(p1=4), dict(step=0), dict(step=3), dict(h=1, p0=1, p1=1), dict(w=1, p0=1, p1=1),
          dict(ldx=32), dict(ldx=44), dict(ldy=32), dict(ldy=44), dict(xns=34 * 48 + 32), dict(xns=35 * 48 + 4),
          dict(yns=47 * 48 + 32), dict(yns=48 * 48 + 4), dict(x=f + 8), dict(y=far + 8), dict(bias=b + 8),
          dict(y=f), dict(y=f + 35 * 48 * 2), dict(y=b)])
    assert lib.vs_lrelu_blur(*[dict(ok, yns=40 * 48)[k] for k in order], None) == INVALID     # (6 x 8 rows needed)
    # the merge: 2 frames of 12 pixels, 40 channels
    order = ("x", "xns", "ldx", "bias", "skip", "sns", "lds", "y", "yns", "ldy", "n", "npix", "c")
    ok = dict(x=f, xns=12 * 48, ldx=48, bias=b, skip=far, sns=12 * 40, lds=40, y=f, yns=12 * 48, ldy=48, n=2, npix=12,
              c=40)
    _all(lib.vs_lrelu_merge, order, ok,
         [dict(x=None), dict(bias=None), dict(y=None), dict(n=0), dict(npix=0), dict(c=0), dict(c=36), dict(ldx=32),
          dict(ldx=44, ldy=44), dict(lds=32), dict(lds=44), dict(ldy=32), dict(xns=11 * 48 + 32, yns=11 * 48 + 32),
          dict(sns=11 * 40 + 32), dict(sns=12 * 40 + 4), dict(x=f + 8, y=f + 8), dict(bias=b + 8), dict(skip=far + 8),
          # y may be x itself and nothing else: another stride on x's pointer, a shifted window, skip, bias
          dict(ldy=56, yns=12 * 56), dict(yns=13 * 48), dict(y=f + 16), dict(y=far), dict(y=b)])
    # Direction: 3 rows, 512 x 20
    order = ("alpha", "lda", "q", "ldq", "out", "ldo", "rows", "d", "m")
    ok = dict(alpha=f, lda=32, q=w, ldq=20, out=far, ldo=512, rows=3, d=512, m=20)
    _all(lib.vs_motion_direction, order, ok,
         [dict(alpha=None), dict(q=None), dict(out=None), dict(rows=0), dict(d=0), dict(m=0), dict(m=33), dict(lda=16),
          dict(ldq=16), dict(ldo=500), dict(alpha=f + 1), dict(q=w + 1), dict(out=far + 1), dict(out=f), dict(out=w)])
