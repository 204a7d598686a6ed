"""The camera adapter's 3x3 convolutions on vs_vae_conv, to the bit, at the adapter's widths -- which the VAE
never reaches: (cin, cout) = (1536, 1536) (the 1.3B dim; cout % 96 == 0: the patch-resident kernel), (5120,
160) and (160, 5120) (the 14B K length and the 14B output width; cout % 96 != 0: the per-tap kernel with three
and with four 32-channel blocks).  One frame of a 4x6 map with bias, the residual and zero padding 1, in the
token layout the adapter uses ([T h w, D] as channels-last with n = T).

In the style of tests/test_vae_conv_exact_gpu.py: x and w in {-1, 0, 1} at density 1/8, bias an integer in
-3..3, the residual an integer in -8..8, so every fp32 partial sum is an integer far below 2^24 whatever the
order, and bf16(acc + bias), bf16(that + res) are exact while within +-256 -- asserted from the float64
reference before any GPU call.  Bar: torch.equal on the bits; the output sits in a sentinel buffer with
guard rows on both sides, which must come back untouched."""
import pytest
import torch
import torch.nn.functional as F

import gpu_util as U

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
H, W = 4, 6


def problem(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)

    def tern(shape):
        r = torch.rand(shape, generator=g)
        return (r < 1 / 16).float() - (r > 15 / 16).float()
    x, w = tern((1, cin, H, W)), tern((cout, cin, 3, 3))
    bias = torch.randint(-3, 4, (cout,), generator=g).float()
    res = torch.randint(-8, 9, (1, cout, H, W), generator=g).float()
    mid = F.conv2d(x.double(), w.double(), bias.double(), padding=1)
    want = mid + res.double()
    assert float(mid.abs().max()) <= 256 and float(want.abs().max()) <= 256      # both roundings exact
    assert float((mid != 0).float().mean()) > 0.5                                 # the sums are not trivial
    return x, w, bias, res, want


@pytest.mark.parametrize("cin,cout", [(1536, 1536), (5120, 160), (160, 5120)])
def test_adapter_conv3x3_exact(cin, cout):
    from vstyler import vae
    x, w, bias, res, want = problem(cin, cout, seed=cin + cout)
    cw = vae.ConvW(w.to(BF16), bias.to(BF16), "cuda")
    assert (cw.cin, cw.cout, cw.k) == (cin, cout, (1, 3, 3))
    rows = lambda t: t[0].permute(1, 2, 0).reshape(H * W, -1).to(BF16).contiguous().cuda()     # [h w, C] token rows
    xr, rr = rows(x), rows(res)
    guard = 8
    buf = U.sentinel(((2 * guard + H * W), cout))
    y = buf[guard:guard + H * W]
    vae.conv(xr.view(1, 1, H, W, cin), cw, (1, H, W), pad=(0, 1, 1), y=y.view(1, 1, H, W, cout),
             res=rr.view(1, 1, H, W, cout))
    torch.cuda.synchronize()
    assert U.untouched(buf[:guard]) and U.untouched(buf[guard + H * W:])
    got = y.float().cpu()
    ref = want[0].permute(1, 2, 0).reshape(H * W, cout).float()
    bad = int((got != ref).sum())
    assert torch.equal(U.bits(y.cpu()), U.bits(ref.to(BF16))), f"{bad} of {ref.numel()} values differ"
