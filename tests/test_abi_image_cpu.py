"""The second ABI table (include/vstyler_image.h, vstyler._lib.SIGNATURES_IMAGE) under the rules the
first one is held to by test_abi.py and test_abi_coverage_cpu.py: every header symbol is exported and has
a ctypes signature; every entry maps to an existing direct test that names it; and the three entries
reject bad arguments before launching (fake aligned pointers, no device)."""
import ast
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# entry -> (file, test function, the name by which the file calls it)
COVERED = {
    "vs_patchify2": ("test_i2v_kernels_gpu.py", "test_patchify2_bit_exact", "K.patchify2("),
    "vs_gelu_erf": ("test_i2v_kernels_gpu.py", "test_gelu_erf_every_bf16", "vs_gelu_erf"),
    "vs_attn_fwd_add": ("test_i2v_kernels_gpu.py", "test_attention_add_equals_attention_then_axpy",
                        "K.attention_add("),
}


def header_symbols():
    src = open(os.path.join(ROOT, "include", "vstyler_image.h")).read()
    return sorted(set(re.findall(r"^\s*(?:const char\*|int)\s+(vs_\w+)\s*\(", src, re.M)))


def test_library_exports_every_image_header_symbol():
    from vstyler import _lib
    lib = _lib.load()
    syms = header_symbols()
    assert syms == sorted(_lib.SIGNATURES_IMAGE), (syms, sorted(_lib.SIGNATURES_IMAGE))
    assert not set(_lib.SIGNATURES_IMAGE) & set(_lib.SIGNATURES)
    for s in syms:
        fn = getattr(lib, s)
        assert fn.argtypes == _lib.SIGNATURES_IMAGE[s], s
    assert lib.vs_abi_version() == 2
    assert len(_lib.OPTIONS) == 13           # no option ids of their own


def test_every_image_entry_has_a_direct_test():
    from vstyler import _lib
    assert set(COVERED) == set(_lib.SIGNATURES_IMAGE)
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


def test_image_entries_reject_bad_arguments_before_launch():
    from vstyler import _lib
    lib = _lib.load()
    f = 1 << 20             # aligned, non-null, never dereferenced: validation fails first
    INVALID, UNSUPPORTED = 1, 3
    # ---- vs_patchify2(x, x_bs, cx, y, y_bs, cy, tokens, ld, batch, frames, height, width, stream)
    ok = dict(x=f, x_bs=0, cx=16, y=f, y_bs=0, cy=20, tok=f, ld=192, b=2, t=2, h=6, w=10)
    bad = [dict(x=None), dict(y=None), dict(tok=None), dict(b=0), dict(t=0), dict(h=0), dict(w=-2), dict(cx=0),
           dict(cy=-1), dict(h=5), dict(w=9), dict(ld=188), dict(ld=136), dict(ld=140), dict(x=f + 2), dict(y=f + 2),
           dict(tok=f + 8), dict(x_bs=-2), dict(y_bs=7)]
    for kw in bad:
        g = dict(ok, **kw)
        rc = lib.vs_patchify2(g["x"], g["x_bs"], g["cx"], g["y"], g["y_bs"], g["cy"], g["tok"], g["ld"], g["b"],
                              g["t"], g["h"], g["w"], None)
        assert rc == INVALID, (kw, rc)
    # ---- vs_gelu_erf(x, out, n, stream)
    assert lib.vs_gelu_erf(None, f, 8, None) == INVALID
    assert lib.vs_gelu_erf(f, None, 8, None) == INVALID
    assert lib.vs_gelu_erf(f, f, 0, None) == INVALID
    assert lib.vs_gelu_erf(f + 1, f, 8, None) == INVALID
    assert lib.vs_gelu_erf(f, f + 1, 8, None) == INVALID
    # ---- vs_attn_fwd_add: vs_attn_fwd's rules, the 31-tile limit, o apart from q / k / v
    far = f + (1 << 24)

    def attn(q=f, k=far, v=2 * far, o=3 * far, b=1, sq=16, skv=16, h=1, hd=128, ldq=128, ldk=128, ldv=128,
             ldo=128, bsq=0, bsk=0, bsv=0, bso=0):
        return lib.vs_attn_fwd_add(q, k, v, o, b, sq, skv, h, hd, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, 1.0, None)
    assert attn(hd=64, ldq=64, ldk=64, ldv=64, ldo=64) == UNSUPPORTED
    assert attn(skv=1985) == UNSUPPORTED
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(b=0), dict(sq=0), dict(skv=0), dict(h=0),
               dict(ldq=130), dict(ldo=64), dict(h=2), dict(bsk=4), dict(bso=-128), dict(o=3 * far + 8), dict(k=far + 2),
               dict(o=f), dict(o=far), dict(o=2 * far)):
        assert attn(**kw) == INVALID, kw
