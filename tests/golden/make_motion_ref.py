"""Writes motion_ref.npz from the reference implementation's diffsynth/models/wan_video_animate_adapter.py.
Usage: python make_motion_ref.py /path/to/wan_video_animate_adapter.py

The reference module is loaded by file path (it needs torch and einops only); no test runs this script.

motion_ref.npz: the reference's Generator(size=64, style_dim=512, motion_dim=20) -- the 256 -> 512 block, three
512 blocks and the 4x4 conv -- with the bf16-valued weights of tests/motion_util.py (motion_weights(64, SEED)) on
three frames: two uint8 64x64 frames (motion_util.face_frames) and the constant -1 frame (byte 0).
  frames        uint8 [3, 64, 64, 3];
  enc_motion    [3, 20], get_motion [3, 512], Q [512, 20]: the float64 module on (u8 * (2 / 255) - 1) in float64;
  get_motion_bf16   [3, 512] (stored as float32): the module cast to bfloat16, literally, on preprocess_image's
                bf16 pixels, on the CPU;
and the sums of absolute values of three weight tensors, so that a drift of the seeded generator shows as such and
not as a parity failure."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import motion_util as M  # noqa: E402

SEED = 41
SIZE = 64
CHECK_KEYS = ("motion_encoder.enc.net_app.convs.0.0.weight", "motion_encoder.enc.fc.4.bias",
              "motion_encoder.dec.direction.weight")


def frames():
    f = M.face_frames(3, SIZE, seed=43)
    f[2] = 0                                    # preprocess_image(0) = -1 exactly
    return f


def main(path):
    spec = importlib.util.spec_from_file_location("reference_wan_video_animate_adapter", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    W = M.motion_weights(SIZE, SEED)
    sd = {k[len(M.PREFIX):]: v for k, v in W.items()}
    u8 = frames()
    gen = mod.Generator(size=SIZE, style_dim=512, motion_dim=20).double().eval()
    gen.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    with torch.no_grad():
        px = u8.permute(0, 3, 1, 2).double() * (2 / 255) + -1
        alpha = gen.enc.enc_motion(px)
        motion = gen.get_motion(px)
        q = gen.dec.direction(None)
        assert torch.equal(px[2], torch.full_like(px[2], -1.0))
        gen16 = mod.Generator(size=SIZE, style_dim=512, motion_dim=20).eval()
        gen16.load_state_dict(sd, strict=True)
        gen16 = gen16.to(torch.bfloat16)
        px16 = u8.permute(0, 3, 1, 2).float().to(torch.bfloat16) * (2 / 255) + -1
        motion16 = gen16.get_motion(px16)
    assert tuple(alpha.shape) == (3, 20) and tuple(motion.shape) == (3, 512) and tuple(q.shape) == (512, 20)
    assert alpha.dtype == motion.dtype == q.dtype == torch.float64 and motion16.dtype == torch.bfloat16
    out = dict(frames=u8.numpy(), enc_motion=alpha.numpy(), get_motion=motion.numpy(), Q=q.numpy(),
               get_motion_bf16=motion16.float().numpy(), seed=np.int64(SEED), size=np.int64(SIZE))
    for k in CHECK_KEYS:
        out["abs_sum." + k] = np.float64(W[k].double().abs().sum().item())
    np.savez_compressed(os.path.join(HERE, "motion_ref.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
