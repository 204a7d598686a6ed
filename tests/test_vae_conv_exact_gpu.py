"""vs_vae_conv in convolution mode, to the bit: the per-tap kernel (vae_conv_kernel) and the
patch-resident one (vae_conv_halo_kernel) against F.conv3d in float64 on the CPU over the explicitly
padded and upsampled input, frames placed by t_mul / t_add / split in plain Python (gpu_util
conv_exact_problem; the preconditions of every case in test_kernel_refs_cpu.py).

Inputs: x and w in {-1, 0, 1} at a seeded density, bias an integer in -3..3, the residual an integer in
-8..8.  Every fp32 partial sum is then an integer far below 2^24, so every summation order (tap-major,
chunk-major, any pipeline depth) gives the same value, and bf16(acc + bias) and bf16(that + res) are exact
while both stay within +-256 -- asserted from the reference alone before any GPU call, as is a non-zero
share of at least one half.  Bar: torch.equal on the bits of the WHOLE y buffer, no tolerance, nothing
excluded: y is a sentinel buffer with ldy = cout rounded up to 4 (8 where the halo kernel's NB = 3
epilogue may run) + 8 pad channels and one guard frame per batch slice behind the last frame, so the
same comparison holds the kernels to what they must leave alone (pad channels, guard frames, frame 0 of
the time convs and of the t_add cases).  Frames of x below t_lo are NaN (both kernels are documented
never to read them), and so is every element of the residual buffer outside the written ones.

The launcher each case reaches (csrc/vae.hip vs_vae_conv / halo_nb), vae_halo = 1 | vae_halo = 0:
  k3 causal, pad (2, 1, 1), n = 2, with bias:
    32 -> 96   17x33 T4 +res | 1x1 T1 | 17x33 T2 t_add 1 +res   launch_conv_halo<3> | launch_conv<3>
    96 -> 192  16x32 T4 t_lo 1 | 15x31 T4 t_lo 2 +res           launch_conv_halo<3>, 2 channel blocks | launch_conv<3>
    384 -> 96  16x32 T1 +res                                    launch_conv_halo<3> | launch_conv<3>
    32 -> 16   17x33 T4 t_lo 1 +res | 15x31 T1 | 17x33 T2 t_add 1    launch_conv_halo<1> | launch_conv<1>
    32 -> 3    17x33 T4 t_lo 2 | 1x1 T4 +res | 16x32 T1         launch_conv_halo<1> | launch_conv<1> (a partial 4-channel group)
    96 -> 64   17x33 T4 t_lo 1 +res | 16x32 T1                  launch_conv<2> (not halo-eligible)
    64 -> 128  15x31 T4 | 1x1 T1 +res                           launch_conv<4>
    96 -> 100  17x33 T4 t_lo 2 +res | 16x32 T1                  launch_conv<4> (100 = 3 x 32 + 4)
  up2 (kt = 1, 3x3, source 9x17 -> 18x34):  96 -> 96 +res  launch_conv_halo<3> | launch_conv<3>;  64 -> 64  launch_conv<2>
  ZeroPad2d + stride (1, 2, 2), 8x12 and 7x11, 64 -> 64:       launch_conv<2>
  time conv stride (2, 1, 1), t_add 1, t = 3, 4, 5, 64 -> 64:  launch_conv<2>
  upsample3d time conv (t_lo 1, t_mul 2, t_add 1, split c):    c = 32: launch_conv<2>, c = 64: launch_conv<4>
  proj (1x1x1 + res into a given y), 96 -> 96:                 launch_conv<3>
  steps1..7 (1x1x1, cin = 32 s, 300 pixels, 96 channels):      launch_conv_px<3, PXB, PRE> for all six (vae_pxb, vae_pre)
"""
import pytest
import torch

import gpu_util as U

pytestmark = pytest.mark.gpu

CASES = U.conv_exact_cases()
GENERAL = [n for n in CASES if n not in U.CONV_STEP_CASES]


def _run(name, opt, **options):
    """One vs_vae_conv launch of the case into a fresh sentinel buffer; returns (problem, y on the CPU)."""
    from vstyler import vae
    p = U.conv_exact_problem(name)
    U.conv_exact_preconditions(p)                     # from the reference alone, before any GPU call
    c = p["case"]
    opt(**options)
    cw = vae.ConvW(p["w"], p["bias"], "cuda")
    assert cw.cin == c["cin"] and cw.cout == c["cout"]
    x = p["x"].cuda()
    y = U.sentinel(tuple(p["want"].shape))
    res = None if p["res"] is None else p["res"].cuda()
    before = U.bits(x).clone()
    vae.conv(x, cw, c["out"], stride=c.get("stride", (1, 1, 1)), pad=c.get("pad", (0, 0, 0)), up2=c.get("up2", False),
             t_lo=c.get("t_lo", 0), y=y, t_mul=c.get("t_mul", 1), t_add=c.get("t_add", 0), split=c.get("split", 0),
             res=res)
    torch.cuda.synchronize()
    assert torch.equal(U.bits(x), before)
    return p, y.cpu()


def _check(name, p, y, what):
    want, written = p["want"], p["written"]
    c = p["case"]
    cout = c["cout"] if not c.get("split") else c["split"]
    diff = U.bits(y) != U.bits(want)
    text = (f"{name} {what}: {int((diff & written).sum())} of {int(written.sum())} written elements differ, "
            f"{int((diff & ~written).sum())} of {int((~written).sum())} others touched")
    # what the call must leave alone, by name: pad channels, the guard frame, the kept frames
    assert U.untouched(y[..., cout:]), text + " (pad channels)"
    assert U.untouched(y[:, -1]), text + " (guard frame)"
    for f in c.get("keep", ()):
        assert U.untouched(y[:, f]), text + f" (frame {f})"
    assert U.untouched(y[~written]), text
    assert torch.equal(U.bits(y), U.bits(want)), text


@pytest.mark.parametrize("halo", [1, 0])
@pytest.mark.parametrize("name", GENERAL)
def test_conv_exact(name, halo, opt):
    """Every conv configuration of the VAE, bit for bit, on the kernel vae_halo selects (the cases that are
    not halo-eligible run the per-tap kernel under both settings)."""
    p, y = _run(name, opt, vae_halo=halo)
    _check(name, p, y, f"vae_halo={halo} (halo NB {U.conv_halo_eligible(p['case']) if halo else 0})")


@pytest.mark.parametrize("name", U.CONV_STEP_CASES)
def test_conv_exact_load_pipeline(name, opt):
    """nsteps = 1..7 K-steps under each (vae_pxb, vae_pre): every residue of the two- and three-stage
    register rotations, the nsteps > 1 / > 2 prologue branches, a ragged 256-pixel tile."""
    for pxb, pre in U.CONV_PIPELINES:
        p, y = _run(name, opt, vae_pxb=pxb, vae_pre=pre)
        _check(name, p, y, f"vae_pxb={pxb} vae_pre={pre}")
