"""Per-episode log files of the ballbot env (reference ballbot_gym/utils/logging.py:9-117).

`save_episode_logs` is a restatement of the reference's function of that name,
with its signature and file formats, as `_save_logs` calls it when an episode
ends (reference ballbot_env.py:673-699, 1027-1034):

  log_dir/term_1.npy, term_2.npy   the directional reward term and the action
                                   penalty, one float32 per step (:102-112)
  log_dir/terrain_seed_history     one "{seed}\\n" line appended per episode,
                                   perlin terrains only (:114-117)
  log_dir/rgbd_log_episode_{k}/    with log_options["cams"]: depth/depth_a_{i}.png
                                   and depth_b_{i}.png, 8-bit grey
                                   (depth * 255).astype(uint8) (:52-100); rgb/ is
                                   created as well, and filled (rbgd_a_{i}.png,
                                   the reference's spelling) when depth_only is
                                   False and the frames carry RGB + depth channels

The reference writes the PNGs with OpenCV; here a small zlib/struct writer does
(`write_png`), so the package needs no image library.

A quirk of the reference that is kept: its env never clears
reward_term_1_hist / reward_term_2_hist (ballbot_env.py:370-372, appended at
:929-937), so term_*.npy holds every step since the env was constructed up to
the latest terminal step, not the last episode alone, and each call overwrites
the files with the longer arrays.  The callers here (BBotSimulation,
BallbotVecEnv.flush_logs) pass such whole histories.
"""
from __future__ import annotations

import os
import struct
import zlib
from typing import Dict, List, Optional

import numpy as np


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path: str, pixels: np.ndarray) -> None:
    """Write uint8 pixels as a PNG: [H, W] 8-bit grey, or [H, W, 3] 8-bit RGB."""
    px = np.ascontiguousarray(pixels)
    if px.dtype != np.uint8 or px.ndim not in (2, 3) or (px.ndim == 3 and px.shape[2] != 3):
        raise ValueError(f"write_png takes uint8 [H, W] or [H, W, 3] pixels, got {px.dtype} {px.shape}")
    h, w = int(px.shape[0]), int(px.shape[1])
    rows = px.reshape(h, -1)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes()  # filter type 0 per scanline
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 0 if px.ndim == 2 else 2, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw, 6))
                + _chunk(b"IEND", b""))


def _depth_plane(frame) -> np.ndarray:
    """A depth frame as [H, W]: the env's channels-first [1, H, W], the reference's [H, W, 1], or [H, W]."""
    a = np.asarray(frame)
    if a.ndim == 3 and a.shape[0] == 1:
        a = a[0]
    elif a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim != 2:
        raise ValueError(f"a depth frame must be [H, W], [1, H, W] or [H, W, 1], got {a.shape}")
    return a


def save_episode_logs(log_dir: str, rgbd_hist_0: List, rgbd_hist_1: List, reward_term_1_hist, reward_term_2_hist,
                      terrain_seed: Optional[int], terrain_type: str, depth_only: bool, log_options: Dict,
                      num_episodes: int, eval_env: bool) -> None:
    """Write one finished episode's logs under log_dir (which exists); see the module docstring.

    reward_term_*_hist are whole histories (the kept quirk: every step since the env was
    constructed, up to this episode's terminal step); the .npy files are overwritten.
    eval_env=True writes nothing (reference logging.py:48-50)."""
    if eval_env:
        return
    if log_options.get("cams", False) and len(rgbd_hist_0) > 0:
        dir_name = f"{log_dir}/rgbd_log_episode_{num_episodes}"
        for d in (dir_name, dir_name + "/depth", dir_name + "/rgb"):
            os.makedirs(d, exist_ok=True)
        for ii in range(len(rgbd_hist_0)):
            for tag, hist in (("a", rgbd_hist_0), ("b", rgbd_hist_1)):
                if depth_only:
                    depth = _depth_plane(hist[ii])
                else:  # [H, W, 4]: RGB then depth (OpenCV's BGR swap and imwrite cancel: the file holds RGB)
                    frame = np.asarray(hist[ii])
                    write_png(f"{dir_name}/rgb/rbgd_{tag}_{ii}.png", (frame[:, :, :3] * 255).astype("uint8"))
                    depth = frame[:, :, 3]
                write_png(f"{dir_name}/depth/depth_{tag}_{ii}.png", (depth * 255).astype("uint8"))
    if log_options.get("reward_terms", False) and len(reward_term_1_hist):
        np.save(log_dir + "/term_1", np.asarray(reward_term_1_hist, dtype=np.float32).reshape(-1))
        np.save(log_dir + "/term_2", np.asarray(reward_term_2_hist, dtype=np.float32).reshape(-1))
    if terrain_type == "perlin" and terrain_seed is not None:
        with open(f"{log_dir}/terrain_seed_history", "a") as fl:
            fl.write(f"{terrain_seed}\n")
