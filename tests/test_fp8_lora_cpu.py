"""Host side of the hot-loaded LoRA on fp8 layers (vs_gemm_fp8_lora, include/vstyler.h; reference
AutoWrappedLinear.forward, diffsynth/vram_management/layers.py:168-182): the new entry point is
exported and validates its arguments before any launch, hotload_lora(fp8_layers="fuse") attaches
adapters to fp8 layers, and the kernels.gemm_fp8 wrapper checks the LoRA operands.  No GPU needed:
invalid calls return VS_E_INVALID up front (fake non-null pointers, never dereferenced)."""
import pytest
import torch

BF16 = torch.bfloat16
FAKE = 1 << 20          # aligned non-null


def _lib():
    from vstyler import _lib
    return _lib, _lib.load()


def test_entry_point_exported_with_signature():
    _l, lib = _lib()
    assert hasattr(lib, "vs_gemm_fp8_lora")
    assert "vs_gemm_fp8_lora" in _l.SIGNATURES
    assert len(_l.SIGNATURES["vs_gemm_fp8_lora"]) == len(_l.SIGNATURES["vs_gemm_fp8"]) + 5
    assert lib.vs_abi_version() == 2


def _call(lib, ep, a8=FAKE, lda=256, sc=FAKE, w8=FAKE, ldw=256, c=FAKE, ldc=8, m=8, n=8, k=256, epi=0,
          a2=FAKE, lda2=64, w2=FAKE, ldw2=64, k2=64):
    return lib.vs_gemm_fp8_lora(a8, lda, sc, w8, ldw, c, ldc, m, n, k, epi, ep, a2, lda2, w2, ldw2, k2, None)


def test_lora_operands_rejected_before_launch():
    _l, lib = _lib()
    ep = _l.VsEpilogue()
    assert _call(lib, ep, k2=48) == 1                       # k2 % 64
    assert _call(lib, ep, k2=-64) == 1
    assert _call(lib, ep, a2=None) == 1                     # k2 > 0 with a null operand
    assert _call(lib, ep, w2=None) == 1
    assert _call(lib, ep, lda2=32) == 1                     # leading dimension below k2
    assert _call(lib, ep, ldw2=32) == 1
    assert _call(lib, ep, lda2=68) == 1                     # not a multiple of 8
    assert _call(lib, ep, w2=FAKE + 8) == 1                 # 16-B alignment of the bases
    assert _call(lib, ep, a2=FAKE + 2) == 1


@pytest.mark.parametrize("k2", [0, 64])
def test_every_vs_gemm_fp8_rule_still_applies(k2):
    """Each argument set vs_gemm_fp8 rejects is rejected by vs_gemm_fp8_lora too, with a valid LoRA
    phase (k2 = 64) and with none (k2 = 0: forwarded)."""
    _l, lib = _lib()
    ep = _l.VsEpilogue()
    bad = [dict(k=192, lda=192, ldw=192),                   # K % 128
           dict(sc=None), dict(a8=None), dict(w8=None), dict(c=None),
           dict(m=0), dict(n=0), dict(k=0),
           dict(n=6, ldc=6),                                # N % 4
           dict(lda=128), dict(ldw=128), dict(ldc=4),       # leading dimensions below the extents
           dict(lda=264), dict(ldw=264), dict(ldc=10),      # lda / ldw % 16, ldc % 4
           dict(a8=FAKE + 8), dict(w8=FAKE + 8), dict(c=FAKE + 4),
           dict(epi=9), dict(epi=3), dict(epi=4)]           # unknown epilogue; residual modes without a residual
    for kw in bad:
        plain = dict(a8=FAKE, lda=256, sc=FAKE, w8=FAKE, ldw=256, c=FAKE, ldc=8, m=8, n=8, k=256, epi=0)
        plain.update(kw)
        assert lib.vs_gemm_fp8(plain["a8"], plain["lda"], plain["sc"], plain["w8"], plain["ldw"], plain["c"],
                               plain["ldc"], plain["m"], plain["n"], plain["k"], plain["epi"], ep, None) == 1, kw
        assert _call(lib, ep, k2=k2, **kw) == 1, kw


def _block_with_one_fp8_layer():
    from vstyler.models import DiTBlock
    blk = DiTBlock(256, 2, 512, device="cpu")
    blk.cross_attn.o.weight_fp8 = torch.zeros(256, 256, dtype=torch.uint8)
    return blk


def _lora(r, scale=1.0):
    lora = {}
    for n in ("self_attn.q", "cross_attn.o"):
        lora[f"{n}.lora_A.default.weight"] = torch.full((r, 256), scale, dtype=BF16)
        lora[f"{n}.lora_B.default.weight"] = torch.full((256, r), scale, dtype=BF16)
    return lora


def test_hotload_fuse_attaches_to_fp8_and_bf16_layers():
    from vstyler.lora import hotload_lora
    blk = _block_with_one_fp8_layer()
    assert hotload_lora(blk, _lora(16), alpha=0.5, fp8_layers="fuse") == 2
    for lin in (blk.self_attn.q, blk.cross_attn.o):             # rank 16 padded to 64, A scaled by alpha
        assert lin.lora_A.shape == (64, 256) and lin.lora_B.shape == (256, 64)
        assert torch.equal(lin.lora_A[:16], torch.full((16, 256), 0.5, dtype=BF16))
        assert not lin.lora_A[16:].any() and not lin.lora_B[:, 16:].any()
    assert blk.cross_attn.o.weight_fp8 is not None
    assert hotload_lora(blk, _lora(96, 2.0), alpha=1.0, fp8_layers="fuse") == 2     # stacked: 64 + 128
    for lin in (blk.self_attn.q, blk.cross_attn.o):
        assert lin.lora_A.shape == (192, 256) and lin.lora_B.shape == (256, 192)
        assert torch.equal(lin.lora_A[:16], torch.full((16, 256), 0.5, dtype=BF16))
        assert torch.equal(lin.lora_A[64:160], torch.full((96, 256), 2.0, dtype=BF16))
        assert torch.equal(lin.lora_B[:, 64:160], torch.full((256, 96), 2.0, dtype=BF16))


def test_hotload_rejects_unknown_fp8_policy_untouched():
    from vstyler.lora import hotload_lora
    blk = _block_with_one_fp8_layer()
    with pytest.raises(ValueError, match="fp8_layers"):
        hotload_lora(blk, _lora(16), fp8_layers="bogus")
    assert getattr(blk.self_attn.q, "lora_A", None) is None and getattr(blk.cross_attn.o, "lora_A", None) is None
    with pytest.raises(NotImplementedError, match="cross_attn.o"):      # the default still refuses, atomically
        hotload_lora(blk, _lora(16))
    assert getattr(blk.self_attn.q, "lora_A", None) is None


def test_hotloaded_fp8_layer_keeps_bf16_rows():
    """A hot-loaded fp8 layer is no fp8 consumer for the LayerNorm in front of it (its LoRA
    down-projection reads the bf16 row), and linear() refuses a quantised activation for it."""
    from vstyler.lora import hotload_lora
    from vstyler.models import Q8, _fp8_consumer, linear
    blk = _block_with_one_fp8_layer()
    assert _fp8_consumer(blk.cross_attn.o)
    hotload_lora(blk, _lora(16), fp8_layers="fuse")
    assert not _fp8_consumer(blk.cross_attn.o)
    q = Q8(torch.zeros(4, 256, dtype=torch.uint8), torch.ones(4))
    with pytest.raises(ValueError, match="hot-loaded"):
        linear(blk.cross_attn.o, q, torch.zeros(4, 256, dtype=BF16), None)


def test_gemm_fp8_wrapper_checks_lora_operands_first():
    """dtype / shape mismatches of a2 / w2 raise ValueError from the tensors' metadata, before any
    operand is required on a device."""
    from vstyler import kernels as K
    M, N, Kd = 8, 12, 128
    a8, w8 = torch.zeros(M, Kd, dtype=torch.uint8), torch.zeros(N, Kd, dtype=torch.uint8)
    sc, out = torch.ones(M), torch.zeros(M, N, dtype=BF16)
    ok_a, ok_w = torch.zeros(M, 64, dtype=BF16), torch.zeros(N, 64, dtype=BF16)
    cases = [(ok_a.float(), ok_w, "a2: expected bfloat16"),
             (ok_a, ok_w.half(), "w2: expected bfloat16"),
             (torch.zeros(M + 1, 64, dtype=BF16), ok_w, "LoRA shape mismatch"),
             (ok_a, torch.zeros(N, 128, dtype=BF16), "LoRA shape mismatch"),
             (ok_a, torch.zeros(N + 4, 64, dtype=BF16), "LoRA shape mismatch"),
             (torch.zeros(M, 32, dtype=BF16), torch.zeros(N, 32, dtype=BF16), "LoRA shape mismatch"),
             (ok_a, None, "go together")]
    for a2, w2, msg in cases:
        with pytest.raises(ValueError, match=msg):
            K.gemm_fp8(a8, sc, w8, out, a2=a2, w2=w2)
