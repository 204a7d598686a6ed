"""The seventh ABI table (include/vstyler_animate.h, vstyler._lib.SIGNATURES_ANIMATE) under the rules the other
tables are held to (test_abi.py, test_abi_coverage_cpu.py, test_abi_control_cpu.py, ...): every header symbol is
exported and has a ctypes signature; the tables are disjoint; every entry maps to an existing direct test that
names it; and the entries reject bad arguments before launching (fake aligned pointers, no device)."""
import ast
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID, UNSUPPORTED = 1, 3

# entry -> (file, test function, the name by which the file calls it)
COVERED = {
    "vs_face_attn": ("test_animate_kernels_gpu.py", "test_face_attn_exact", "K.face_attn("),
    "vs_head_rmsnorm": ("test_animate_kernels_gpu.py", "test_head_rmsnorm_rows", "K.head_rmsnorm("),
    "vs_ln_silu": ("test_animate_kernels_gpu.py", "test_ln_silu_every_bf16", "K.ln_silu("),
}


def header_symbols():
    src = open(os.path.join(ROOT, "include", "vstyler_animate.h")).read()
    return sorted(set(re.findall(r"^\s*(?:const char\*|int)\s+(vs_\w+)\s*\(", src, re.M)))


def test_library_exports_every_animate_header_symbol():
    from vstyler import _lib
    lib = _lib.load()
    syms = header_symbols()
    assert syms == sorted(_lib.SIGNATURES_ANIMATE), (syms, sorted(_lib.SIGNATURES_ANIMATE))
    for other in (_lib.SIGNATURES, _lib.SIGNATURES_IMAGE, _lib.SIGNATURES_CLIP, _lib.SIGNATURES_SEG,
                  _lib.SIGNATURES_CONTROL, _lib.SIGNATURES_VAE22):
        assert not set(_lib.SIGNATURES_ANIMATE) & set(other)
    for s in syms:
        fn = getattr(lib, s)
        assert fn.argtypes == _lib.SIGNATURES_ANIMATE[s], s
    assert lib.vs_abi_version() == 2
    assert len(_lib.OPTIONS) == 13           # no option ids of their own
    assert ctypes.sizeof(_lib.VsEpilogue) == 72


def test_every_animate_entry_has_a_direct_test():
    from vstyler import _lib
    assert set(COVERED) == set(_lib.SIGNATURES_ANIMATE)
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


def _all(fn, order, ok, bad, want=INVALID):
    for kw in bad:
        g = dict(ok, **kw)
        rc = fn(*[g[k] for k in order], None)
        assert rc == want, (fn.__name__, kw, rc)


def test_animate_entries_reject_bad_arguments_before_launch():
    from vstyler import _lib
    lib = _lib.load()
    f = 1 << 20             # aligned, non-null, never dereferenced: validation fails first
    far = 1 << 30           # a second buffer that overlaps nothing
    inf, nan = float("inf"), float("nan")
    order = ("q", "ldq", "k", "v", "ldkv", "bs", "o", "ldo", "wq", "b", "rpb", "h", "hd", "fr", "tpf", "nk", "off",
             "eps", "scale")
    # 2 samples x 18 rows, 2 heads, 3 frames x 6 tokens, 5 keys; K | V the halves of [.., 512] rows
    ok = dict(q=f, ldq=256, k=far, v=far + 512, ldkv=512, bs=15 * 512, o=f, ldo=256, wq=far + (1 << 20), b=2, rpb=18,
              h=2, hd=128, fr=3, tpf=6, nk=5, off=0, eps=1e-6, scale=0.0884)
    _all(lib.vs_face_attn, order, ok,
         [dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(wq=None), dict(b=0), dict(rpb=0), dict(h=0),
          dict(hd=0), dict(fr=0), dict(tpf=0), dict(nk=0), dict(nk=9), dict(off=-1), dict(eps=-1.0), dict(eps=nan),
          dict(scale=inf), dict(scale=nan), dict(ldq=248), dict(ldq=260), dict(ldo=248), dict(ldo=260),
          dict(ldkv=248), dict(ldkv=516), dict(bs=14 * 512 + 248), dict(bs=15 * 512 + 4), dict(bs=-512),
          dict(q=f + 8), dict(k=far + 8), dict(v=far + 520), dict(o=f + 8), dict(wq=far + (1 << 20) + 8),
          # o may be q itself and nothing else: another stride on q's pointer, a shifted window, K, V or wq
          dict(ldo=264), dict(o=f + 512), dict(o=far), dict(o=far + 512), dict(o=far + (1 << 20))])
    _all(lib.vs_face_attn, order, ok, [dict(hd=64), dict(hd=256)], want=UNSUPPORTED)
    order = ("x", "ldx", "rows", "h", "hd", "w", "eps")
    ok = dict(x=f, ldx=5120, rows=105, h=40, hd=128, w=far, eps=1e-6)
    _all(lib.vs_head_rmsnorm, order, ok,
         [dict(x=None), dict(w=None), dict(rows=0), dict(h=0), dict(hd=0), dict(eps=-1.0), dict(eps=nan),
          dict(ldx=5112), dict(ldx=5124), dict(x=f + 8), dict(w=far + 8)])
    _all(lib.vs_head_rmsnorm, order, ok, [dict(hd=64)], want=UNSUPPORTED)
    order = ("x", "ldx", "out", "ldo", "rows", "dim", "norm", "eps")
    ok = dict(x=f, ldx=1024, out=far, ldo=1024, rows=308, dim=1024, norm=1, eps=1e-6)
    _all(lib.vs_ln_silu, order, ok,
         [dict(x=None), dict(out=None), dict(rows=0), dict(dim=0), dict(dim=1020), dict(dim=8200), dict(eps=-1.0),
          dict(eps=nan), dict(ldx=1016), dict(ldx=1028), dict(ldo=1016), dict(ldo=1028), dict(x=f + 8),
          dict(out=far + 8), dict(out=f + 2048), dict(out=f, ldo=1032)])
