"""Writes animate_ref.npz and animate_keys.json from the reference implementation's
diffsynth/models/wan_video_animate_adapter.py.
Usage: python make_animate_ref.py /path/to/wan_video_animate_adapter.py

The reference module is loaded by file path (it needs torch and einops only); no test runs this script.

animate_ref.npz, in float64 with the bf16-valued weights of tests/animate_util.py (adapter_weights(256, 2, 6,
in_dim=32)) and bf16-valued inputs:
  face_encoder   FaceEncoder(in_dim=32, hidden_dim=256, num_heads=4) on a (1, 9, 32) input -> (1, 3, 5, 256);
  face_block     FaceBlock(256, 2) (fuser block 0) on x (1, 4 * 6, 256) with that motion tensor behind a zero
                 frame (1, 4, 5, 256) -> (1, 24, 256);
and the sums of absolute values of three weight tensors, so that a drift of the seeded generator shows as such
and not as a parity failure.

animate_keys.json: the parameter names and shapes of the reference's WanAnimateAdapter() (built on the meta
device: 138 tensors), the key set a Wan2.2-Animate-14B file adds to the I2V DiT's."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import animate_util as A  # noqa: E402

SEED = 31
CHECK_KEYS = ("face_encoder.conv1_local.conv.weight", "face_adapter.fuser_blocks.0.linear1_kv.weight",
              "face_adapter.fuser_blocks.0.q_norm.weight")


def inputs():
    g = torch.Generator().manual_seed(SEED)
    motion = torch.randn((1, 9, 32), generator=g).to(torch.bfloat16).double()
    x = torch.randn((1, 24, 256), generator=g).to(torch.bfloat16).double()
    return motion, x


def sub(W, prefix):
    return {k[len(prefix):]: v.double() for k, v in W.items() if k.startswith(prefix)}


def main(path):
    spec = importlib.util.spec_from_file_location("reference_wan_video_animate_adapter", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    W = A.adapter_weights(256, 2, 6, in_dim=32, seed=SEED)
    enc = mod.FaceEncoder(in_dim=32, hidden_dim=256, num_heads=4).double().eval()
    enc.load_state_dict(sub(W, "face_encoder."), strict=True)
    blk = mod.FaceBlock(256, 2).double().eval()
    blk.load_state_dict(sub(W, "face_adapter.fuser_blocks.0."), strict=True)
    motion, x = inputs()
    with torch.no_grad():
        tok = enc(motion)
        mv = torch.cat([torch.zeros_like(tok[:, :1]), tok], dim=1)
        res = blk(x, mv)
    assert tuple(tok.shape) == (1, 3, 5, 256) and tuple(res.shape) == (1, 24, 256)
    assert tok.dtype == res.dtype == torch.float64
    out = dict(face_encoder=tok.numpy(), face_block=res.numpy(), seed=np.int64(SEED))
    for k in CHECK_KEYS:
        out["abs_sum." + k] = np.float64(W[k].double().abs().sum().item())
    np.savez_compressed(os.path.join(HERE, "animate_ref.npz"), **out)
    with torch.device("meta"):
        full = mod.WanAnimateAdapter()
    keys = {k: list(v.shape) for k, v in full.state_dict().items()}
    assert len(keys) == 138, len(keys)
    with open(os.path.join(HERE, "animate_keys.json"), "w") as f:         # one tensor per line
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(keys[n])}" for n in sorted(keys)) + "\n}\n")


if __name__ == "__main__":
    main(sys.argv[1])
