"""Writes vae22_ref.npz: the float64 output of the reference implementation's VideoVAE38_ (the Wan2.2 VAE,
diffsynth/models/wan_video_vae.py) -- its own chunked, feature-cache encode and decode -- for the tiny
configuration and the seeded weights of tests/vae22_util.py.
Usage: python make_vae22_ref.py /path/to/wan_video_vae.py

The reference module is loaded by file path (it needs torch, einops and tqdm only); no test runs this
script.  encode: a (1, 3, 9, 32, 48) video (chunks of 1, 4, 4 frames); decode: a (1, 48, 3, 2, 3) latent (one
latent frame per chunk).  Inputs and weights are bf16 values widened to float64.  The sums of absolute values
of three weight tensors are stored too, so that a drift of the seeded generator shows as such and not as a
parity failure."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import vae22_util as U  # noqa: E402

SEED = 31
CHECK_KEYS = ("encoder.conv1.weight", "decoder.upsamples.1.upsamples.3.time_conv.weight", "conv2.bias")


def inputs():
    g = torch.Generator().manual_seed(SEED)
    video = (torch.rand((1, 3, 9, 32, 48), generator=g) * 2 - 1).to(torch.bfloat16).double()
    latent = torch.randn((1, 48, 3, 2, 3), generator=g).to(torch.bfloat16).double()
    return video, latent


def main(path):
    spec = importlib.util.spec_from_file_location("reference_wan_video_vae", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = U.TINY_VAE22
    W = U.random_vae22_weights(cfg, SEED)
    model = mod.VideoVAE38_(dim=cfg["dim"], z_dim=cfg["z_dim"], dec_dim=cfg["dec_dim"]).double().eval()
    missing = model.load_state_dict({k: v.double() for k, v in W.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    scale = [torch.tensor(U.MEAN), 1.0 / torch.tensor(U.STD)]
    video, latent = inputs()
    with torch.no_grad():
        mu = model.encode(video, scale)
        rec = model.decode(latent, scale)
    assert tuple(mu.shape) == (1, 48, 3, 2, 3) and tuple(rec.shape) == (1, 3, 9, 32, 48)
    assert mu.dtype == rec.dtype == torch.float64
    out = dict(encode=mu.numpy(), decode=rec.numpy(), seed=np.int64(SEED))
    for k in CHECK_KEYS:
        out["abs_sum." + k] = np.float64(W[k].double().abs().sum().item())
    np.savez_compressed(os.path.join(HERE, "vae22_ref.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
