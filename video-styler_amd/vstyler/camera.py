"""Camera control's host side (diffsynth/models/wan_video_camera_controller.py:46-59, 77-107, 150-206;
WanVideoUnit_FunCameraControl, diffsynth/pipelines/wan_video_new.py:806-823).

The host builds F small matrices -- the trajectory's per-frame intrinsics and relative camera-to-world
poses -- in numpy float64 and casts them to float32 where the reference does; the per-pixel Pluecker rays
and their grouping in fours are one kernel (kernels.camera_rays), which writes the adapter's input
[1, 24, T, H, W] directly.
"""
import numpy as np
import torch

from . import kernels as K

BF16 = torch.bfloat16

# entry layout: [_, fx, fy, cx, cy, _, _, w2c 3x4 row major]; the reference's default camera
DEFAULT_ORIGIN = (0, 0.532139961, 0.946026558, 0.5, 0.5, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
DEFAULT_SPEED = 1 / 54
DIRECTIONS = ("Left", "Right", "Up", "Down", "LeftUp", "LeftDown", "RightUp", "RightDown", "In", "Out")
# the entry a direction word moves, and its sign (the reference's indices into the 19-entry row)
_MOVES = (("Left", 9, 1.0), ("Right", 9, -1.0), ("Up", 13, 1.0), ("Down", 13, -1.0), ("In", 18, -1.0), ("Out", 18, 1.0))
POSE_ASPECT = 1280 / 720      # the aspect ratio the trajectory's intrinsics are given for


def camera_coordinates(direction, length, speed=DEFAULT_SPEED, origin=DEFAULT_ORIGIN):
    """`length` entries: the origin, then each the previous one moved by `speed` along every direction
    word contained in `direction` (accumulated step by step, as the reference does)."""
    if direction not in DIRECTIONS:
        raise ValueError(f"camera_control_direction must be one of {DIRECTIONS}, got {direction!r}")
    if origin is None:
        origin = DEFAULT_ORIGIN
    if len(origin) != 19:
        raise ValueError(f"camera_control_origin has 19 entries, got {len(origin)}")
    out = [list(origin)]
    while len(out) < length:
        cur = list(out[-1])
        for word, idx, sign in _MOVES:
            if word in direction:
                cur[idx] += sign * speed
        out.append(cur)
    return out


def camera_matrices(direction, length, height, width, speed=DEFAULT_SPEED, origin=DEFAULT_ORIGIN):
    """(intrinsics float32 [F, 4] = (fx W, fy H, cx W, cy H), c2w float32 [F, 3, 4]): the focal length
    rescaled from the pose aspect ratio to width / height, and every camera's pose relative to the first
    (frame 0: the identity)."""
    entries = camera_coordinates(direction, length, speed, origin)
    fx = [e[1] for e in entries]
    fy = [e[2] for e in entries]
    if POSE_ASPECT > width / height:
        fx = [height * POSE_ASPECT * f / width for f in fx]
    else:
        fy = [width / POSE_ASPECT * f / height for f in fy]
    intr = np.asarray([[fx[i] * width, fy[i] * height, e[3] * width, e[4] * height] for i, e in enumerate(entries)],
                      dtype=np.float32)
    w2c = []
    for e in entries:
        m = np.eye(4)
        m[:3, :] = np.array(e[7:]).reshape(3, 4)
        w2c.append(m)
    rel = [np.eye(4)] + [w2c[0] @ np.linalg.inv(m) for m in w2c[1:]]
    return intr, np.ascontiguousarray(np.array(rel, dtype=np.float32)[:, :3, :])


def control_camera_latents_input(direction, num_frames, height, width, speed=DEFAULT_SPEED, origin=DEFAULT_ORIGIN,
                                 device="cuda"):
    """WanVideoUnit_FunCameraControl's control_camera_latents_input [1, 24, T, height, width] bf16, T =
    (num_frames + 3) / 4: channel c 4 + j of latent frame t is ray component c of pixel frame
    max(0, 4 t + j - 3)."""
    if num_frames % 4 != 1 or height % 16 or width % 16:
        raise ValueError(f"camera control: num_frames 4k + 1 and height, width multiples of 16, got {num_frames} "
                         f"frames at {height}x{width}")
    intr, c2w = camera_matrices(direction, num_frames, height, width, speed, origin)
    out = torch.empty((24, (num_frames + 3) // 4, height, width), device=device, dtype=BF16)
    K.camera_rays(torch.from_numpy(intr).to(device), torch.from_numpy(c2w).to(device), out)
    return out[None]
