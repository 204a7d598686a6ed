"""Writes camera_plucker.npz: the fp32 output of the reference implementation's
SimpleAdapter.process_camera_coordinates (diffsynth/models/wan_video_camera_controller.py) for the cases
below.  Usage: python make_camera_plucker.py /path/to/wan_video_camera_controller.py

The reference module is loaded by file path (it needs torch, numpy and einops only); no test runs this
script.  Each case is 5 frames at 16x32; with the default origin every moment channel is exactly zero, so
the third case -- an origin with a rotation and a translation -- is the one that exercises o x d."""
import importlib.util
import math
import os
import sys

import numpy as np

FRAMES, HEIGHT, WIDTH = 5, 16, 32


def rotated_origin():
    """fx, fy, cx, cy of the default camera; w2c = a rotation (0.3 rad about y, then 0.2 rad about x) with
    the translation (0.3, -0.2, 0.5)."""
    a, b = 0.3, 0.2
    ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    m = np.concatenate([rx @ ry, np.array([[0.3], [-0.2], [0.5]])], axis=1)
    return (0, 0.532139961, 0.946026558, 0.5, 0.5, 0, 0) + tuple(float(v) for v in m.reshape(-1))


CASES = {
    "left": dict(direction="Left", speed=1 / 54, origin=None),
    "rightdown": dict(direction="RightDown", speed=1 / 54, origin=None),
    "leftup_rot": dict(direction="LeftUp", speed=0.05, origin=rotated_origin()),
}


def main(path):
    spec = importlib.util.spec_from_file_location("reference_camera_controller", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for name, c in CASES.items():
        p = mod.SimpleAdapter.process_camera_coordinates(None, c["direction"], FRAMES, HEIGHT, WIDTH, c["speed"],
                                                         c["origin"])
        assert tuple(p.shape) == (FRAMES, HEIGHT, WIDTH, 6) and str(p.dtype) == "torch.float32"
        out[name] = p.numpy()
        out[name + "_origin"] = np.asarray(c["origin"] if c["origin"] is not None else [], dtype=np.float64)
        out[name + "_speed"] = np.float64(c["speed"])
        out[name + "_direction"] = np.asarray(c["direction"])
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "camera_plucker.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
