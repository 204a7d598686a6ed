"""vs_vae_conv at the motion encoder's geometries, to the bit: for the (cin, cout) of every real ResBlock the 3x3
stride-1 pad-1 conv (conv1, on an odd 9 x 11 input), the 3x3 stride-2 pad-0 conv (conv2, on 7 x 7), the 1x1 skip
conv, and the 4x4 pad-0 conv on a 4 x 4 input -- none of which the VAE's own exact tests reach (2-D convs on n
frames with t_in = 1, no bias, cin up to 512 with 3x3, a 4x4 kernel).

Inputs as in test_vae_conv_exact_gpu.py: x and w in {-1, 0, 1} at a density chosen so that every output is an
integer within +-256 (asserted from the float64 reference before any GPU call): every fp32 partial sum is exact in
any order and bf16(acc) is exact.  n = 2 frames whose stride x_ns is larger than the frame (NaN between them).  Bar:
torch.equal on the bits of the whole sentinel-filled y buffer (ldy = cout + 8: the pad channels stay untouched)."""
import pytest
import torch
import torch.nn.functional as F

import gpu_util as U

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

BLOCKS = [(32, 64), (64, 128), (128, 256), (256, 512), (512, 512)]
CASES = {}
for ci, co in BLOCKS:
    CASES[f"conv1_{ci}"] = dict(cin=ci, cout=ci, k=3, stride=1, pad=1, hw=(9, 11))
    CASES[f"conv2_{ci}_{co}"] = dict(cin=ci, cout=co, k=3, stride=2, pad=0, hw=(7, 7))
    CASES[f"skip_{ci}_{co}"] = dict(cin=ci, cout=co, k=1, stride=1, pad=0, hw=(5, 3))
CASES["last_512"] = dict(cin=512, cout=512, k=4, stride=1, pad=0, hw=(4, 4))


def problem(name):
    c = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    K = c["cin"] * c["k"] ** 2
    d = min(1.0, (1600.0 / K) ** 0.5)               # sum variance K d^2 <= 1600: |sum| stays far below 256
    h, w = c["hw"]

    def tern(shape):
        return (torch.randint(-1, 2, shape, generator=g) * (torch.rand(shape, generator=g) < d)).float()
    x = tern((2, c["cin"], h, w))
    wt = tern((c["cout"], c["cin"], c["k"], c["k"]))
    want = F.conv2d(x.double(), wt.double(), stride=c["stride"], padding=c["pad"])
    assert want.abs().max() <= 256 and (want != 0).float().mean() > 0.5
    return c, x, wt, want.permute(0, 2, 3, 1).contiguous()      # channels-last [n, ho, wo, cout]


@pytest.mark.parametrize("name", list(CASES))
def test_motion_conv_exact(name):
    from vstyler import _lib, vae
    c, x, wt, want = problem(name)
    h, w = c["hw"]
    ho, wo, cin, cout = want.shape[1], want.shape[2], c["cin"], c["cout"]
    frame = h * w * cin
    xbuf = torch.full((2, frame + 64), float("nan"), dtype=BF16)
    xbuf[:, :frame] = x.permute(0, 2, 3, 1).reshape(2, frame).to(BF16)
    xbuf = xbuf.cuda()
    cw = vae.ConvW(wt, None, "cuda")
    assert cw.cin == cin and tuple(cw.w.shape) == (cout, c["k"] ** 2 * cin)
    ldy = cout + 8
    y = U.sentinel((2, ho * wo + 1, ldy))                       # one guard pixel row per frame
    p = _lib.VsConv3d()
    p.x, p.x_zs, p.x_ns, p.ldx = xbuf.data_ptr(), 0, xbuf.stride(0), cin
    p.n, p.t_in, p.h_in, p.w_in, p.cin = 2, 1, h, w, cin
    p.kt, p.kh, p.kw = 1, c["k"], c["k"]
    p.st, p.sh, p.sw = 1, c["stride"], c["stride"]
    p.pt, p.ph, p.pw = 0, c["pad"], c["pad"]
    p.up2, p.t_lo = 0, 0
    p.t_out, p.h_out, p.w_out = 1, ho, wo
    p.w, p.w_zs, p.ldw = cw.w.data_ptr(), 0, cw.w.shape[1]
    p.bias, p.cout = None, cout
    p.y, p.y_zs, p.y_ns, p.ldy = y.data_ptr(), 0, y.stride(0), ldy
    p.t_mul, p.t_add, p.split, p.out_f32, p.alpha = 1, 0, 0, 0, 1.0
    p.res, p.nz = None, 1
    before = U.bits(xbuf).clone()
    _lib.check(_lib.load().vs_vae_conv(p, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(U.bits(xbuf), before)
    y = y.cpu()
    got = y[:, :ho * wo, :cout].reshape(2, ho, wo, cout)
    diff = got.float() != want.float()
    text = f"{name}: {int(diff.sum())} of {diff.numel()} elements differ"
    assert U.untouched(y[:, :, cout:]), text + " (pad channels touched)"
    assert U.untouched(y[:, ho * wo:]), text + " (guard row touched)"
    assert torch.equal(U.bits(got), U.bits(want.to(BF16))), text
