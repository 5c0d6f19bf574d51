"""BallbotVecEnv: N ballbot envs stepped by one HIP launch per env.step.

Batched replacement for `BBotSimulation` (ballbot_gym/envs/ballbot_env.py:60)
as driven by SB3's VecEnv (ballbot_rl/training/train.py:60-120): the physics
(`mujoco.mj_step`, ballbot_env.py:912), observation packing (:771-811), the
reward plugin (:929-937) and termination (:982-1017) all run in the fused
step kernel behind the C-ABI (include/ballbot_mi355x.h).  Tensors live on the
GPU; `step` takes and returns torch tensors on `device`.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional, Sequence

import numpy as np
import torch

from .. import _native as N

OBS_KEYS = ("actions", "angular_vel", "motor_state", "orientation", "vel")  # sorted, as the policy reads them


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class BallbotVecEnv:
    """Vectorised ballbot env on one GPU.

    Args mirror BBotSimulation (ballbot_env.py:157-231) plus `num_envs`,
    `device`, `precision` ("fp32" | "fp64") and the terrain bank size.

    Terrain seeds follow the reference's per-reset draw r_seed =
    _np_random.integers(0, 10000) (ballbot_env.py:505-510), drawn on the GPU
    from numpy's PCG64 per env (bb_set_terrain_rng).  By default env i draws
    from np_random(seed + i): SB3 seeds the training VecEnv that way
    (VecEnv.seed(seed), then reset(seed=seed+i) in learn(); gymnasium's
    Env.reset replaces _np_random, ballbot_env.py:596; train.py:126-141).
    `stream_seeds` gives env i np_random(stream_seeds[i]) (an eval VecEnv:
    seed + N_ENVS + i, train.py:90-97); `shared_stream=True` puts every env on
    np_random(seed).  `seed(s)` re-seeds env i to np_random(s + i) at the next
    reset(), as SB3's VecEnv.seed does.  `n_terrains`: the draws per generator
    whose terrains a host-generated bank holds (perlin default: the whole
    10^4-seed space, generated on the GPU).  `terrain_draws`: an explicit list
    of terrain seeds that every env walks instead (a replayed draw log).

    `disable_cameras=False` adds the onboard cameras' keys (rgbd_0, rgbd_1,
    relative_image_timestamp), rendered every `cam_every` steps and at a reset: depth
    frames (1, H, W) by default, RGB-D frames (4, H, W) -- R, G, B in [0, 1] plus depth --
    with env_config["camera"]["disable_rgb"] = False (`cam_channels` 4, `rgbd`
    f32[N, 2, 4, H, W], `depth` a view of its D planes; the colour is defined in DESIGN.md §5).

    `render_mode="rgb_array"` enables render(): env 0's world-view frame as a numpy
    array (ballbot_env.py:1077-1135).  render_view() renders any envs into a device
    tensor and needs no render_mode.  Nothing is rendered unless one of them is called.

    `log_options` (with env_config's `logging` section on top, ballbot_env.py:214-218)
    turns on the reference's per-episode log files (_save_logs, :673-699): keys
    `reward_terms` (term_1.npy / term_2.npy), `terrain_seeds` (terrain_seed_history),
    `envs` (local indices of the envs that log; None: all), `dir` (env i logs under
    dir/env_{first_env + i:05d}/; default: a fresh temporary directory) and `cams`
    (refused: frame dumps are BBotSimulation's).  Both switches need the built-in
    directional reward.  The files are current after flush_logs() -- see the
    "per-episode logs" section below.  With every switch off (the default) no launch,
    buffer or file is added.
    """

    metadata = {"render_modes": ["rgb_array"], "render_fps": 30}
    render_mode = None

    def __init__(
        self,
        num_envs: int,
        device: str | torch.device = "cuda:0",
        reward_config: Optional[Dict[str, Any]] = None,
        terrain_config: Optional[Dict[str, Any]] = None,
        env_config: Optional[Dict[str, Any]] = None,
        max_ep_steps: Optional[int] = None,
        seed: int = 0,
        precision: str = "fp64",
        n_terrains: Optional[int] = None,
        auto_reset: bool = True,
        disable_cameras: bool = True,
        stream_seeds: Optional[Sequence[int]] = None,
        terrain_draws: Optional[Sequence[int]] = None,
        shared_stream: bool = False,
        terrain_slots: Optional[int] = None,
        reward_compat: str = "reference",
        opt_timestep: Optional[float] = None,
        opt_disableflags: int = 0,
        log_options: Optional[Dict[str, Any]] = None,
        first_env: int = 0,
        render_mode: Optional[str] = None,
    ):
        from .config import params_from_configs

        if render_mode is not None and render_mode not in self.metadata["render_modes"]:
            raise ValueError(f"Invalid render_mode: {render_mode}. Supported modes: {self.metadata['render_modes']}")
        if render_mode is not None:  # the class attribute stays None: nothing renders unless asked
            self.render_mode = render_mode
        self._log_on = False  # the per-episode logs (log_options), set up after the first reset
        if not torch.cuda.is_available():
            raise RuntimeError("BallbotVecEnv needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"BallbotVecEnv runs on a GPU device, got {self.device}")
        self.num_envs = int(num_envs)
        self.auto_reset = bool(auto_reset)
        # depth cameras (ballbot_env.py:211-290; camera: height/width/frame_rate/disable_rgb).
        # The reference defaults to cameras on; the batched env defaults to off (the
        # proprio hot path) -- pass disable_cameras=False for rgbd_0/rgbd_1 obs.
        self.cameras = not disable_cameras
        cam = ((env_config or {}).get("camera", {}) or {})
        self.cam_h, self.cam_w = int(cam.get("height", 64)), int(cam.get("width", 64))
        fr = float(cam.get("frame_rate", 90))
        self.cam_every = int(np.ceil((1.0 / fr) / float(opt_timestep or 0.002)))  # effective_camera_frame_rate (ballbot_env.py:389-411)
        # camera.disable_rgb false: rgbd_0 / rgbd_1 are (4, H, W), RGB in [0, 1] plus depth (bb_render_rgbd)
        self.cam_channels = 4 if self.cameras and not cam.get("disable_rgb", True) else 1
        self.terrain_config = terrain_config or {"type": "flat", "config": {}}
        self.reward_config = reward_config or {"type": "directional", "config": {"target_direction": [0.0, 1.0]}}
        p, self.reward_obj, self._host_reward = params_from_configs(self.reward_config, env_config, max_ep_steps,
                                                                    precision, seed, reward_compat=reward_compat)
        from .config import reward_error

        # reward_compat="reference": a DistanceReward raises at the first step, as
        # in the reference env (its obs lacks pos2d); "fused": the kernel computes it
        self._reward_error = reward_error(self.reward_obj, reward_compat)
        self.first_env = int(first_env)  # global id of env 0 (a rank's block, distributed.env_shard)
        self.log_options = self._log_config(log_options, env_config, p)
        # mjModel.opt overrides (physics invariant tests): timestep and MuJoCo's
        # mjDSBL_PASSIVE / mjDSBL_GRAVITY bits (_native.DSBL_*); the reference never sets them
        p.opt_timestep = float(opt_timestep or 0.0)
        p.opt_disableflags = int(opt_disableflags)
        self.opt_timestep = float(opt_timestep or 0.002)
        self.max_ep_steps = int(p.max_ep_steps)
        self.precision = "fp64" if p.fp64 else "fp32"
        self._params = p
        self._seed = int(seed)
        self._n_terrains_arg = n_terrains
        self._shared_stream = bool(shared_stream)
        self._pending_seeds: Optional[list] = None
        self._graphs = 0  # HIP graphs captured over this handle (capture_step, the trainer's rollout graph)
        self._h = None
        if terrain_slots is not None:  # host-driven terrains (load_terrain + assign_terrain), e.g. BBotSimulation
            from .config import TerrainPlan, terrain_size_z

            plan = TerrainPlan([-1] * int(terrain_slots), None, None, False, terrain_size_z(self.terrain_config))
            self._install(plan, generate=False)
        else:
            self._install(self._plan(stream_seeds, terrain_draws))
        n, dev = self.num_envs, self.device
        self.obs = torch.zeros(n, N.NOBS, dtype=torch.float32, device=dev)
        self.terminal_obs = torch.zeros(n, N.NOBS, dtype=torch.float32, device=dev)
        self.reward = torch.zeros(n, dtype=torch.float32, device=dev)
        self.done = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.pos2d = torch.zeros(n, 2, dtype=torch.float32, device=dev)
        if self.cameras:
            if self.cam_channels == 4:
                if "bb_render_rgbd" not in N.EXPORTS:
                    raise RuntimeError("this build has no bb_render_rgbd (camera.disable_rgb: false)")
                self.rgbd = torch.ones(n, 2, 4, self.cam_h, self.cam_w, dtype=torch.float32, device=dev)
                self.depth = self.rgbd[:, :, 3]  # a view: the D plane, for the depth image's readers
            else:
                self.depth = torch.ones(n, 2, self.cam_h, self.cam_w, dtype=torch.float32, device=dev)
            self.rel_ts = torch.zeros(n, dtype=torch.float32, device=dev)
        from .. import spaces

        # SB3 VecEnv / gymnasium attributes (ballbot_env.py:235-256)
        self.action_space = spaces.action_space()
        self.observation_space = spaces.observation_space({"h": self.cam_h, "w": self.cam_w}, self.cam_channels,
                                                          not self.cameras)
        self._pending_actions: Optional[torch.Tensor] = None
        self.reset()  # the first reset: draw 0 of every env's generator
        self._log_alloc()

    # ------------------------------------------------------------ terrain bank
    def _plan(self, stream_seeds=None, terrain_draws=None):
        from .config import gpu_perlin_plan, terrain_plan

        gp = gpu_perlin_plan(self.terrain_config, self._n_terrains_arg, self._seed, self.num_envs, stream_seeds,
                             terrain_draws, shared=self._shared_stream)
        if gp is not None:
            return gp[0]
        return terrain_plan(self.terrain_config, self._n_terrains_arg, self._seed, self.num_envs, stream_seeds,
                            draws=terrain_draws, shared=self._shared_stream)

    def _install(self, plan, generate: bool = True) -> None:
        """A handle whose bank holds the plan's terrains, with its generators
        (bb_set_terrain_rng) or draw table (bb_set_terrain_stream) installed."""
        from .config import bank_fields, perlin_cfg

        perlin = self._gpu_perlin()
        bank = []
        if generate and not perlin:
            bank = [(h, plan.size_z) for h in bank_fields(self.terrain_config, plan)]
        p = self._params
        p.n_terrains = len(plan.seeds)
        L = N.lib()
        if self._h is not None:
            if self._graphs:
                raise RuntimeError(
                    f"{self._graphs} HIP graph(s) were captured over this env's handle, and the new terrain "
                    "generators' draws are not in its bank: regenerating the bank needs a new handle, which "
                    "those graphs would not follow (re-seed before capturing, or with a bank that covers the "
                    "new draws, e.g. perlin's whole seed space)")
            L.bb_destroy(self._h)
            self._h = None
        h = C.c_void_p()
        N.check(L.bb_create(self.num_envs, self.device.index or 0, C.byref(p), C.byref(h)), "bb_create")
        self._h = h
        for i, (data, size_z) in enumerate(bank):
            arr = np.ascontiguousarray(data, dtype=np.float32)
            N.check(L.bb_set_hfield(h, i, arr.ctypes.data_as(C.POINTER(C.c_float)), float(size_z)), "bb_set_hfield")
        if generate and perlin:
            sd = np.ascontiguousarray(plan.seeds, dtype=np.int32)
            N.check(L.bb_generate_perlin(h, 0, len(sd), sd.ctypes.data_as(C.POINTER(C.c_int32)),
                                         C.byref(perlin_cfg(self.terrain_config)), float(plan.size_z)),
                    "bb_generate_perlin")
        self.terrain_plan = plan
        self.terrain_seeds = plan.seeds
        self.n_terrains = p.n_terrains
        # any terrain with relief: bb_step routes through the predictor (route 0) on such banks
        self.relief = (generate and perlin) or any(float(np.max(data)) > 0.0 for data, _ in bank)
        self._set_draws(plan)

    def _gpu_perlin(self) -> bool:
        tc = self.terrain_config
        return tc.get("type", "flat") == "perlin" and (tc.get("config", {}) or {}).get("seed") is None

    def _set_draws(self, plan) -> None:
        L, ip = N.lib(), C.POINTER(C.c_int32)
        if plan.stream_seeds is not None:  # one PCG64 per env on the device
            words = np.ascontiguousarray(plan.rng_words())
            ss = None if plan.seed_slot is None else np.ascontiguousarray(plan.seed_slot, dtype=np.int32)
            N.check(L.bb_set_terrain_rng(self._h, words.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         None if ss is None else ss.ctypes.data_as(ip)), "bb_set_terrain_rng")
        elif plan.streams is not None:  # an explicit draw table
            st = np.ascontiguousarray(plan.streams, dtype=np.int32)
            es = None if plan.env_stream is None else np.ascontiguousarray(plan.env_stream, dtype=np.int32)
            N.check(L.bb_set_terrain_stream(self._h, st.ctypes.data_as(ip), st.shape[0], st.shape[1],
                                            None if es is None else es.ctypes.data_as(ip)), "bb_set_terrain_stream")

    def _reseed(self, stream_seeds) -> None:
        """Put env i on np_random(stream_seeds[i]) from its next reset on (its draw
        counter restarts).  The generators are rewritten in place (bb_set_terrain_rng), so
        HIP graphs captured before this draw from them at replay.  A bank that lacks the new
        generators' first draws would need a new handle: refused once graphs exist."""
        from .config import stream_draws, terrain_plan

        plan = self.terrain_plan
        if plan.stream_seeds is None and plan.streams is None:
            return  # one fixed terrain (flat or a config seed): nothing is drawn
        stream_seeds = [int(x) for x in stream_seeds]
        if len(stream_seeds) != self.num_envs:
            raise ValueError(f"need one seed per env ({self.num_envs}), got {len(stream_seeds)}")
        k = self._n_terrains_arg or 8
        need = {int(v) for s in dict.fromkeys(stream_seeds) for v in stream_draws(s, k)}
        if plan.stream_seeds is not None and plan.covers(need):
            from .config import TerrainPlan

            new = TerrainPlan(plan.seeds, stream_seeds, plan.seed_slot, plan.full, plan.size_z, seedless=plan.seedless)
            self.terrain_plan = new
            self._set_draws(new)
            return
        self._install(self._plan(stream_seeds))

    # --------------------------------------------------------------------- api
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self, mask: Optional[torch.Tensor] = None):
        """Reset every env (mask None) or the masked ones -> (obs, {}).  A full
        reset first applies the seeds of seed(), as SB3's VecEnv.reset passes
        seed + i to env i's reset (then forgets them)."""
        seed_log = self._log_on and self._log_seeds and not torch.cuda.is_current_stream_capturing()
        if seed_log:  # the episodes finished so far belong to the draws (and generators) before this reset
            self.flush_logs()
        if mask is None and self._pending_seeds is not None:
            pending, self._pending_seeds = self._pending_seeds, None
            self._reseed(pending)
        m = None if mask is None else mask.to(device=self.device, dtype=torch.uint8).contiguous()
        N.check(N.lib().bb_reset(self._h, _ptr(m), _ptr(self.obs), self._stream()), "bb_reset")
        if self.cameras:
            self._render(force=m is None)
        if seed_log:
            self._log_rebase()
        return self.obs, {}

    def _render(self, force: bool) -> None:
        if self.cam_channels == 4:  # the D plane comes with the colour: the depth kernel is not launched as well
            N.check(N.lib().bb_render_rgbd(self._h, _ptr(self.rgbd), _ptr(self.rel_ts), None, self.cam_h, self.cam_w,
                                           self.cam_every, int(force), self._stream()), "bb_render_rgbd")
            return
        N.check(N.lib().bb_render_depth(self._h, _ptr(self.depth), _ptr(self.rel_ts), self.cam_h, self.cam_w,
                                        self.cam_every, int(force), self._stream()), "bb_render_depth")

    def render_depth(self, force: bool = True) -> torch.Tensor:
        """Depth images [N, 2, H, W] of cam_0/cam_1 at the current state (linear depth, clipped to 1 m).
        With camera.disable_rgb false this renders the RGB-D frames and returns their D planes (a view)."""
        if not self.cameras:
            raise RuntimeError("cameras are disabled (BallbotVecEnv(..., disable_cameras=False))")
        self._render(force)
        return self.depth

    def render_rgbd(self, force: bool = True) -> torch.Tensor:
        """RGB-D images [N, 2, 4, H, W] of cam_0/cam_1 at the current state: R, G, B in [0, 1] (the
        colour defined in DESIGN.md §5) and the linear depth clipped to 1 m."""
        if not self.cameras or self.cam_channels != 4:
            raise RuntimeError("RGB-D cameras are off (BallbotVecEnv(..., disable_cameras=False, "
                               "env_config={'camera': {'disable_rgb': False}}))")
        self._render(force)
        return self.rgbd

    def render_view(self, env_ids=None, height: int = 640, width: int = 480, *, azimuth: float = 90.0,
                    elevation: float = -20.0, distance: float = 2.5, lookat_offset=(0.0, 0.0, 0.2),
                    fovy: float = 45.0, out: Optional[torch.Tensor] = None,
                    ids_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """World-view RGB frames uint8 [k, H, W, 3] of the envs `env_ids` (None: env 0; a sequence or an
        int32 device tensor, any order, duplicates allowed) at the current state, from MuJoCo's free
        camera tracking each env's base (bb_render_view; the image is defined in DESIGN.md §5).
        `out` (uint8 [k, H, W, 3]) and `ids_out` (int8 [k, H, W]: 0 none, 1 ground, 2 ball, 3 tower,
        4-5 sticks, 6-8 wheels) are contiguous device tensors written in place.  Enqueued on the
        current stream; the first call with more views than any before allocates scratch."""
        if env_ids is None:
            env_ids = [0]
        if isinstance(env_ids, torch.Tensor):
            ids = env_ids.to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
        else:
            ids = torch.as_tensor(np.asarray(env_ids, np.int32).reshape(-1)).to(self.device)
        k, H, W = int(ids.numel()), int(height), int(width)
        if H < 1 or W < 1:
            raise ValueError(f"render_view: frame size {H}x{W} must be at least 1x1")
        if out is None:
            out = torch.empty(k, H, W, 3, dtype=torch.uint8, device=self.device)
        for t, shape, dt, name in ((out, (k, H, W, 3), torch.uint8, "out"), (ids_out, (k, H, W), torch.int8, "ids_out")):
            if t is not None and (tuple(t.shape) != shape or t.dtype != dt or t.device != self.device
                                  or not t.is_contiguous()):
                raise ValueError(f"render_view: {name} must be a contiguous {dt} tensor of shape {shape} on {self.device}")
        cfg = N.ViewCfg(H, W, float(fovy), float(azimuth), float(elevation), float(distance),
                        (C.c_float * 3)(*[float(x) for x in lookat_offset]))
        N.check(N.lib().bb_render_view(self._h, _ptr(ids), k, C.byref(cfg), _ptr(out), _ptr(ids_out), self._stream()),
                "bb_render_view")
        return out

    def render(self):
        """gymnasium's render() in rgb_array mode: env 0's world-view frame, uint8 numpy [640, 480, 3]
        (the reference's _video_renderer_size, ballbot_env.py:1077-1135)."""
        if self.render_mode != "rgb_array":
            raise RuntimeError('render() needs BallbotVecEnv(..., render_mode="rgb_array")')
        return self.render_view()[0].cpu().numpy()

    def step(self, actions: torch.Tensor):
        """One env.step for all envs: returns (obs[N,15], reward[N], terminated[N], truncated[N], info)."""
        if actions.device != self.device or actions.dtype != torch.float32 or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        if actions.shape != (self.num_envs, 3):
            raise ValueError(f"actions must have shape ({self.num_envs}, 3), got {tuple(actions.shape)}")
        N.check(N.lib().bb_step(self._h, _ptr(actions), _ptr(self.obs), _ptr(self.reward), _ptr(self.done),
                                _ptr(self.terminal_obs), _ptr(self.pos2d), int(self.auto_reset), self._stream()),
                "bb_step")
        if self.cameras:  # envs whose counter hit the frame interval (incl. auto-resets) re-render
            self._render(force=False)
        self._record(self.terminal_obs, self.done, 1)
        if self._reward_error:  # after mj_step, as the reference's reward call (ballbot_env.py:912, 929)
            raise ValueError(self._reward_error)
        terminated = (self.done & N.DONE_TERMINATED) != 0
        info = {"done_flags": self.done, "terminal_observation": self.terminal_obs, "pos2d": self.pos2d,
                "failure": (self.done & N.DONE_FAILURE) != 0}
        reward = self.reward
        if self._host_reward is not None:
            reward = self._plugin_reward(info["failure"])
        return self.obs, reward, terminated, torch.zeros_like(terminated), info

    def step_flags(self, actions: torch.Tensor):
        """env.step without the derived tensors, for the batched trainer's
        rollout: -> (obs[N,15], reward[N], done_flags[N] uint8, BB_DONE_* bits).
        Same launch and buffers as step()."""
        if self._host_reward is not None:
            obs, reward, _, _, info = self.step(actions)
            return obs, reward, info["done_flags"]
        if self._reward_error:
            raise ValueError(self._reward_error)
        if actions.device != self.device or actions.dtype != torch.float32 or not actions.is_contiguous() \
                or actions.shape != (self.num_envs, 3):
            raise ValueError(f"actions must be a contiguous float32 ({self.num_envs}, 3) tensor on {self.device}")
        N.check(N.lib().bb_step(self._h, _ptr(actions), _ptr(self.obs), _ptr(self.reward), _ptr(self.done),
                                _ptr(self.terminal_obs), _ptr(self.pos2d), int(self.auto_reset), self._stream()),
                "bb_step")
        if self.cameras:
            self._render(force=False)
        self._record(self.terminal_obs, self.done, 1)
        return self.obs, self.reward, self.done

    def capture_step(self, actions: torch.Tensor) -> "torch.cuda.CUDAGraph":
        """Capture one env.step (routing, fast/full step kernels on the env's two
        streams, depth cameras) reading `actions` as ONE HIP graph; replay() then
        steps every env with whatever `actions` holds (one launch per rollout step)."""
        if actions.shape != (self.num_envs, 3) or actions.dtype != torch.float32 or not actions.is_contiguous():
            raise ValueError("capture_step needs a contiguous float32 [num_envs, 3] action buffer")
        if self._reward_error:
            raise ValueError(self._reward_error)
        graph = torch.cuda.CUDAGraph()
        self.note_graph_capture()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        torch.cuda.synchronize(self.device)
        with torch.cuda.graph(graph, stream=side):
            self._step_launch(actions)
        torch.cuda.synchronize(self.device)
        return graph

    def note_graph_capture(self) -> None:
        """Record that a HIP graph holding this env's handle exists (it lives as long as the env):
        a re-seed that would need a new handle then raises instead of leaving the graph stale.
        A graph captured over an env that logs holds the log history's address: the history can no
        longer move, so it must have been sized before (reserve_log_rows)."""
        self._graphs += 1
        if self._log_on:
            self._log_pinned = True

    def _step_launch(self, actions: torch.Tensor) -> None:
        N.check(N.lib().bb_step(self._h, _ptr(actions), _ptr(self.obs), _ptr(self.reward), _ptr(self.done),
                                _ptr(self.terminal_obs), _ptr(self.pos2d), int(self.auto_reset), self._stream()),
                "bb_step")
        if self.cameras:
            self._render(force=False)
        self._record(self.terminal_obs, self.done, 1)

    def step_multi(self, actions: torch.Tensor, out: Optional[dict] = None) -> dict:
        """K env.steps of all envs in ONE launch for actions known in advance
        (bb_step_multi; open-loop sequences such as random-action benchmarks):
        actions [K, N, 3] -> {"obs" [K,N,15], "reward" [K,N], "done" [K,N] uint8,
        "terminal_obs" [K,N,15], "pos2d" [K,N,2]}, identical to K step() calls
        (auto-reset, counters and terrain draws included).  `out` (a dict
        returned before, same K) is refilled instead of allocating.  The env's
        obs/reward/done buffers are not updated; cameras are not rendered."""
        if self.cameras:
            raise RuntimeError("step_multi does not render the depth cameras; step() does")
        if self._host_reward is not None:
            raise RuntimeError("step_multi needs a built-in reward (a host plugin runs per step())")
        if self._reward_error:
            raise ValueError(self._reward_error)
        if actions.device != self.device or actions.dtype != torch.float32 or not actions.is_contiguous() \
                or actions.dim() != 3 or actions.shape[1:] != (self.num_envs, 3):
            raise ValueError(f"actions must be a contiguous float32 (K, {self.num_envs}, 3) tensor on {self.device}")
        k = int(actions.shape[0])
        if out is None or out["reward"].shape[0] != k:
            n = self.num_envs
            out = {"obs": torch.empty(k, n, 15, device=self.device), "reward": torch.empty(k, n, device=self.device),
                   "done": torch.empty(k, n, dtype=torch.uint8, device=self.device),
                   "terminal_obs": torch.empty(k, n, 15, device=self.device),
                   "pos2d": torch.empty(k, n, 2, device=self.device)}
        N.check(N.lib().bb_step_multi(self._h, _ptr(actions), k, _ptr(out["obs"]), _ptr(out["reward"]),
                                      _ptr(out["done"]), _ptr(out["terminal_obs"]), _ptr(out["pos2d"]),
                                      int(self.auto_reset), self._stream()), "bb_step_multi")
        self._record(out["terminal_obs"], out["done"], k)
        return out

    def step_multi_raw(self, actions: torch.Tensor, obs: torch.Tensor, reward: torch.Tensor,
                       done: torch.Tensor, terminal_obs: Optional[torch.Tensor] = None,
                       pos2d: Optional[torch.Tensor] = None) -> None:
        """Launch-only bb_step_multi (benchmarking): caller-owned [K, N, ...] outputs
        (terminal obs / pos2d optional; an env that logs needs the terminal obs)."""
        if self._log_on and terminal_obs is None:
            raise ValueError("this env records per-episode logs (log_options): step_multi_raw needs terminal_obs")
        N.check(N.lib().bb_step_multi(self._h, _ptr(actions), int(actions.shape[0]), _ptr(obs), _ptr(reward),
                                      _ptr(done), _ptr(terminal_obs), _ptr(pos2d), int(self.auto_reset),
                                      self._stream()), "bb_step_multi")
        self._record(terminal_obs, done, int(actions.shape[0]))

    def check(self) -> None:
        """Wait for the env's stream and raise if a bb_step_multi relief-pair launch ended on its
        wall-clock budget (bb_check).  The fault is sticky: step(), step_multi() and rollouts raise
        too, without a sync, until a full reset() clears it."""
        N.check(N.lib().bb_check(self._h, self._stream()), "bb_check")

    def run_rollout(self, args) -> None:
        """One whole PPO rollout in one launch (bb_rollout; args: _native.RolloutArgs
        filled by the trainer).  Built-in rewards only; the cameras are not rendered."""
        if self.cameras:
            raise RuntimeError("bb_rollout steps the proprio policy; the camera policy rolls out per step")
        if self._host_reward is not None:
            raise RuntimeError("bb_rollout needs a built-in reward (a host plugin runs per step())")
        if self._reward_error:
            raise ValueError(self._reward_error)
        if self._log_on and self._log_recording and not (args.buf_terminal_obs and args.buf_flags):
            raise RuntimeError("this env records per-episode logs (log_options): the rollout needs "
                               "buf_terminal_obs and buf_flags ([T][n][15] float32, [T][n] uint8)")
        N.check(N.lib().bb_rollout(self._h, C.byref(args), self._stream()), "bb_rollout")
        if args.buf_terminal_obs and args.buf_flags:
            self._record(C.c_void_p(args.buf_terminal_obs), C.c_void_p(args.buf_flags), int(args.n_steps))

    def run_pid_rollout(self, args) -> None:
        """K steps of the PID balance loop in one launch (bb_pid_rollout; args: _native.PIDRolloutArgs
        filled by BatchedPID.rollout / balance).  Built-in rewards only; the cameras are not rendered."""
        if self.cameras:
            raise RuntimeError("bb_pid_rollout does not render the cameras; act() and step() do")
        if self._host_reward is not None:
            raise RuntimeError("bb_pid_rollout needs a built-in reward (a host plugin runs per step())")
        if self._reward_error:
            raise ValueError(self._reward_error)
        if "bb_pid_rollout" not in N.EXPORTS:
            raise RuntimeError("this build has no bb_pid_rollout")
        if self._log_on and self._log_recording and not (args.buf_terminal_obs and args.buf_flags):
            raise RuntimeError("this env records per-episode logs (log_options): the PID rollout needs "
                               "buf_terminal_obs and buf_flags ([K][n][15] float32, [K][n] uint8)")
        N.check(N.lib().bb_pid_rollout(self._h, C.byref(args), int(self.auto_reset), self._stream()), "bb_pid_rollout")
        if args.buf_terminal_obs and args.buf_flags:
            self._record(C.c_void_p(args.buf_terminal_obs), C.c_void_p(args.buf_flags), int(args.n_steps))

    def step_async_raw(self, actions: torch.Tensor, full_outputs: bool = False) -> None:
        """Launch-only step (graph capture / benchmarking): no derived tensors;
        full_outputs: also the terminal obs and pos2d buffers (an env that logs always
        keeps the terminal obs: its recorder reads them)."""
        N.check(N.lib().bb_step(self._h, _ptr(actions), _ptr(self.obs), _ptr(self.reward), _ptr(self.done),
                                _ptr(self.terminal_obs) if full_outputs or self._log_on else None,
                                _ptr(self.pos2d) if full_outputs else None, int(self.auto_reset), self._stream()),
                "bb_step")
        self._record(self.terminal_obs, self.done, 1)

    def _plugin_reward(self, failure: torch.Tensor) -> torch.Tensor:
        """Reward of a custom plugin, in the reference's float32 order
        (ballbot_env.py:929-937, 1019-1020): plugin(obs) * scale + action penalty
        (the kernel's reward for BB_REWARD_NONE), then + survival bonus unless failed.
        The plugin sees this step's observation (before any auto-reset) and pos2d."""
        f32 = np.float32
        hb = getattr(type(self._host_reward), "has_batched", None)
        if hb is not None and hb():  # device path: one call, no host sync
            st = {k: self.terminal_obs[:, 3 * i:3 * i + 3] for i, k in enumerate(OBS_KEYS)}
            st["pos2d"] = self.pos2d
            v = torch.as_tensor(self._host_reward.batched(st), device=self.device).to(torch.float32).reshape(-1)
            if v.shape[0] != self.num_envs:
                raise ValueError(f"{type(self._host_reward).__name__}.batched returned {v.shape[0]} rewards "
                                 f"for {self.num_envs} envs")
        else:  # compatibility path: BaseReward.__call__(state) per env on the host
            obs = self.terminal_obs.cpu().numpy()
            pos = self.pos2d.cpu().numpy()
            out = np.zeros(self.num_envs, dtype=f32)
            for i in range(self.num_envs):
                state = split_obs(obs[i])
                state["pos2d"] = pos[i]
                out[i] = f32(self._host_reward(state))
            v = torch.from_numpy(out).to(self.device)
        r = v * f32(self._params.reward_scale) + self.reward
        return torch.where(failure, r, r + f32(self._params.survival_bonus))

    # ------------------------------------------------------- per-episode logs
    # The reference env writes, when an episode ends (_save_logs, ballbot_env.py:673-699):
    # term_1.npy / term_2.npy (the reward's two terms per step) and one line of
    # terrain_seed_history.  Here a recorder kernel (bb_reward_terms) follows every step
    # launch on the same stream: it appends the steps' [K][n][2] terms to a device-resident
    # history and keeps, per env, the step of its last terminal row and its count of
    # finished episodes.  Nothing is copied to the host per step; flush_logs() writes the
    # files.  The one deliberate difference from the reference: the files are current after
    # flush_logs() (close() flushes; the trainer flushes at every update boundary), not
    # after every step.
    def _log_config(self, log_options, env_config, p) -> Dict[str, Any]:
        """log_options (keys reward_terms, cams, terrain_seeds, envs, dir) with env_config's
        `logging` section on top, as the reference overrides them (ballbot_env.py:214-218)."""
        opts: Dict[str, Any] = {"reward_terms": False, "cams": False, "terrain_seeds": False, "envs": None,
                                "dir": None}
        opts.update(log_options or {})
        opts.update((env_config or {}).get("logging", {}) or {})
        if opts["cams"]:
            raise ValueError("log_options['cams']: per-episode frame dumps are a single-env feature "
                             "(BBotSimulation(log_options={'cams': True})); the batched env writes no frames")
        if (opts["reward_terms"] or opts["terrain_seeds"]) and p.reward_kind != N.REWARD_DIRECTIONAL:
            what = "reward_terms" if opts["reward_terms"] else "terrain_seeds"
            raise ValueError(f"log_options[{what!r}] needs the built-in directional reward, got "
                             f"{type(self.reward_obj).__name__}: the reference env logs the terms of that reward "
                             "only (ballbot_env.py:929-937), and the recorder that also counts the finished "
                             "episodes (bb_reward_terms) computes them")
        if opts["envs"] is not None:
            envs = sorted({int(i) for i in opts["envs"]})
            if envs and not (0 <= envs[0] and envs[-1] < self.num_envs):
                raise ValueError(f"log_options['envs'] must be indices in [0, {self.num_envs}), got {opts['envs']}")
            opts["envs"] = envs
        return opts

    LOG_ROWS0 = 256  # first allocation of the term history, in steps (doubled as it fills)

    def _log_alloc(self) -> None:
        o = self.log_options
        self._log_terms, self._log_seeds = bool(o["reward_terms"]), bool(o["terrain_seeds"])
        self._log_recording = True
        self._log_pinned = False  # a captured graph holds the history's address
        self.log_dir = None
        if not (self._log_terms or self._log_seeds):
            return
        import os
        import tempfile

        n, dev = self.num_envs, self.device
        self.log_dir = str(o["dir"]) if o["dir"] else tempfile.mkdtemp(prefix="ballbot_env_logs_")
        os.makedirs(self.log_dir, exist_ok=True)
        self._log_envs = list(range(n)) if o["envs"] is None else list(o["envs"])
        self._log_idx = None if o["envs"] is None else torch.tensor(self._log_envs, dtype=torch.int64, device=dev)
        # recorder state (bb_reward_terms): [0:n] last terminal step + 1, [n:2n] finished episodes,
        # [2n] steps recorded, [2n+1] kernel scratch
        self._log_book = torch.zeros(2 * n + 2, dtype=torch.int64, device=dev)
        self._log_hist = torch.zeros(self.LOG_ROWS0, n, 2, dtype=torch.float32, device=dev)
        self._log_rows = 0  # host mirror of book[2n]
        self._log_flushed = 0  # ... at the last flush_logs()
        self._log_written = np.zeros(n, np.int64)  # finished episodes already in the files
        self._log_draw_base = np.zeros(n, np.int64)  # terrain draw index of an env's episode k = base + k
        self._log_draws: Dict[int, np.ndarray] = {}
        self._log_on = True

    def reserve_log_rows(self, rows: int, recapture: bool = False) -> None:
        """Room for `rows` more recorded steps in the device-resident term history.  Growing
        moves the history (a stream-ordered copy).  A HIP graph captured over this env holds its
        address, so reserve before capturing; recapture=True grows anyway -- the caller then
        drops the graphs it captured over this env and captures them again."""
        if not self._log_on:
            return
        need, cap = self._log_rows + int(rows), int(self._log_hist.shape[0])
        if need <= cap:
            return
        if torch.cuda.is_current_stream_capturing() or (self._log_pinned and not recapture):
            raise RuntimeError(f"the log history holds {cap} steps and {need} are needed, but a captured HIP graph "
                               "holds its address: call reserve_log_rows() before capturing")
        new = torch.zeros(max(need, 2 * cap), self.num_envs, 2, dtype=torch.float32, device=self.device)
        new[:cap].copy_(self._log_hist)
        self._log_hist = new
        self._log_pinned = False

    def log_rows_free(self) -> int:
        """Steps the term history still has room for before it must grow (reserve_log_rows)."""
        return int(self._log_hist.shape[0]) - self._log_rows if self._log_on else 1 << 62

    def set_log_recording(self, on: bool) -> None:
        """Pause / resume the recorder (steps taken while paused never enter the history)."""
        self._log_recording = bool(on)

    def note_log_rows(self, rows: int) -> None:
        """Tell the env that a replayed graph (capture_step, the trainer's rollout graph)
        recorded `rows` more steps: the recorder's launches inside it advanced the device
        counter, and flush_logs() sizes its copy from the host's count."""
        if self._log_on:
            self._log_rows += int(rows)

    def _record(self, terminal_obs, flags, k: int) -> None:
        """Launch the recorder over k steps' rows (terminal obs [k][n][15], done bytes [k][n];
        tensors or raw device pointers) on the current stream."""
        if not (self._log_on and self._log_recording):
            return
        self.reserve_log_rows(k)
        tp = terminal_obs if isinstance(terminal_obs, C.c_void_p) else _ptr(terminal_obs)
        fp = flags if isinstance(flags, C.c_void_p) else _ptr(flags)
        N.check(N.lib().bb_reward_terms(self._h, tp, fp, int(k), _ptr(self._log_hist), int(self._log_hist.shape[0]),
                                        _ptr(self._log_book), self._stream()), "bb_reward_terms")
        if not torch.cuda.is_current_stream_capturing():  # a captured launch runs at replay (note_log_rows)
            self._log_rows += int(k)

    def log_state(self):
        """(terms [rows][N][2] float32 device view of the history, last terminal step + 1 per env
        int64[N], finished episodes per env int64[N]) -- waits for the stream."""
        if not self._log_on:
            raise RuntimeError("this env records no per-episode logs (log_options)")
        book = self._log_book.cpu().numpy()
        n = self.num_envs
        rows = min(int(book[2 * n]), int(self._log_hist.shape[0]))
        return self._log_hist[:rows], book[:n].copy(), book[n:2 * n].copy()

    def _log_seed(self, e: int, k: int):
        """Terrain seed of env e's draw k (its k-th reset since its generator was installed)."""
        plan = self.terrain_plan
        if plan.stream_seeds is not None:
            from .config import stream_draws

            s = int(plan.stream_seeds[e])
            d = self._log_draws.get(s)
            if d is None or len(d) <= k:
                d = self._log_draws[s] = stream_draws(s, max(2 * (k + 1), 16))
            return int(d[k])
        if plan.streams is not None:  # the terrain_draws table (wraps around, as on the device)
            row = 0 if plan.env_stream is None else int(plan.env_stream[e])
            return int(plan.seeds[int(plan.streams[row][k % plan.streams.shape[1]])])
        return int(plan.seeds[0]) if plan.seeds and int(plan.seeds[0]) >= 0 else None  # a fixed config seed

    def flush_logs(self) -> None:
        """Bring the log files up to date: one wait for the stream, then, for every logged env
        whose count of finished episodes advanced since the last flush,
        <dir>/env_{global id:05d}/term_1.npy and term_2.npy -- every step since construction up
        to the env's last terminal step (the reference never clears its term histories,
        ballbot_env.py:370-372) -- and one terrain_seed_history line per newly finished episode
        (perlin terrains).  Files are written by utils.logging.save_episode_logs."""
        if not self._log_on or self._h is None:
            return
        import os

        from ..utils.logging import save_episode_logs

        if self._log_rows == self._log_flushed and not self._log_pinned:
            return  # nothing was recorded since the last flush (replayed graphs may not have reported)
        n, cap = self.num_envs, int(self._log_hist.shape[0])
        stream = torch.cuda.current_stream(self.device)
        book_h = torch.empty(2 * n + 2, dtype=torch.int64, pin_memory=True)
        book_h.copy_(self._log_book, non_blocking=True)

        def fetch(rows: int):
            src = self._log_hist[:rows] if self._log_idx is None else self._log_hist[:rows].index_select(
                1, self._log_idx)
            out = torch.empty(src.shape, dtype=torch.float32, pin_memory=True)
            out.copy_(src, non_blocking=True)
            return out

        rows = min(self._log_rows, cap)
        hist_h = fetch(rows) if self._log_terms and rows else None
        stream.synchronize()
        book = book_h.numpy()
        recorded = int(book[2 * n])
        if recorded > cap:
            import warnings

            warnings.warn(f"the log history holds {cap} steps but {recorded} were recorded (graph replays past "
                          "reserve_log_rows): the steps past it are missing from term_*.npy")
        if self._log_terms and min(recorded, cap) > rows:  # a graph replay nobody reported (note_log_rows)
            rows = min(recorded, cap)
            hist_h = fetch(rows)
            stream.synchronize()
        self._log_rows = self._log_flushed = max(self._log_rows, recorded)
        terms = None if hist_h is None else hist_h.numpy()
        ttype = self.terrain_config.get("type", "flat")
        for col, e in enumerate(self._log_envs):
            done_eps = int(book[n + e])
            first = int(self._log_written[e])
            if done_eps <= first:
                continue
            env_dir = os.path.join(self.log_dir, f"env_{self.first_env + e:05d}")
            os.makedirs(env_dir, exist_ok=True)
            last = min(int(book[e]), rows)
            for ep in range(first, done_eps):
                final = ep == done_eps - 1  # the .npy files are overwritten: only the last write stays
                seed = self._log_seed(e, ep + int(self._log_draw_base[e])) if self._log_seeds else None
                save_episode_logs(env_dir, [], [], terms[:last, col, 0] if (final and terms is not None) else [],
                                  terms[:last, col, 1] if (final and terms is not None) else [], seed, ttype, True,
                                  {"cams": False, "reward_terms": self._log_terms and final}, ep, False)
            self._log_written[e] = done_eps

    def _log_rebase(self) -> None:
        """After a reset() by the caller: the envs' draw counters moved without an episode ending."""
        _, draws = self.env_terrain()
        self._log_draw_base = draws.astype(np.int64) - 1 - self._log_written

    # ------------------------------------------------- SB3 VecEnv interface
    def step_async(self, actions) -> None:
        """VecEnv.step_async: remember the actions (torch [N,3] or numpy); step_wait runs the step."""
        self._pending_actions = torch.as_tensor(actions, dtype=torch.float32, device=self.device)

    def step_wait(self):
        """VecEnv.step_wait -> (obs dict of [N,...] tensors, rewards [N], dones [N] bool, infos list).

        dones = terminated (the reference never truncates); done envs were reset
        in the same launch, their last observation is infos[i]["terminal_observation"]
        (SB3's convention).  The per-env info dicts are host objects: the batched
        trainer reads the tensors of step() instead."""
        if self._pending_actions is None:
            raise RuntimeError("step_wait() without step_async()")
        obs, reward, term, trunc, info = self.step(self._pending_actions)
        self._pending_actions = None
        done = term | trunc
        d_h = done.cpu().numpy()
        fail = info["failure"].cpu().numpy()
        p2 = info["pos2d"].cpu().numpy()
        tob = info["terminal_observation"].cpu().numpy()
        infos = []
        for i in range(self.num_envs):
            inf = {"TimeLimit.truncated": False, "failure": bool(fail[i]), "success": False, "pos2d": p2[i]}
            if d_h[i]:
                inf["terminal_observation"] = split_obs(tob[i])
            infos.append(inf)
        return self.obs_dict(obs), reward, done, infos

    def seed(self, seed: Optional[int] = None):
        """VecEnv.seed (SB3 2.x): env i re-seeds to np_random(seed + i) at the next
        reset() -- the terrain generator, as reset(seed=seed+i) replaces the
        reference env's _np_random (ballbot_env.py:596) -- and the action space is
        seeded.  seed None: a random base, as SB3 draws one.  -> the seeds."""
        if seed is None:
            seed = int(np.random.randint(0, np.iinfo(np.uint32).max, dtype=np.uint32))
        self._pending_seeds = [int(seed) + i for i in range(self.num_envs)]
        self.action_space.seed(seed)
        return list(self._pending_seeds)

    def load_terrain(self, slot: int, seed: Optional[int]) -> None:
        """Generate the terrain of `seed` (the registered plugin, or the GPU perlin
        generator) into bank slot `slot` (terrain_slots mode; ballbot_env.py:501-513)."""
        from .config import _gen_chunk, perlin_cfg

        L = N.lib()
        size_z = self.terrain_plan.size_z
        if self._gpu_perlin() and seed is not None:
            sd = np.array([int(seed)], np.int32)
            N.check(L.bb_generate_perlin(self._h, int(slot), 1, sd.ctypes.data_as(C.POINTER(C.c_int32)),
                                         C.byref(perlin_cfg(self.terrain_config)), float(size_z)),
                    "bb_generate_perlin")
        else:
            arr = np.ascontiguousarray(_gen_chunk(self.terrain_config, [seed], N.HF_N)[0], dtype=np.float32)
            N.check(L.bb_set_hfield(self._h, int(slot), arr.ctypes.data_as(C.POINTER(C.c_float)), float(size_z)),
                    "bb_set_hfield")
        self.terrain_seeds[int(slot)] = seed if seed is not None else -1

    def terrain_rng(self):
        """(uint64[N][5] device generators in pcg64_words form (None without generators), int32[N] terrain seed of
        each env's last device draw, -1 before the first)."""
        gen = self.terrain_plan.stream_seeds is not None
        w = np.zeros((self.num_envs, 5), np.uint64) if gen else None
        s = np.zeros(self.num_envs, np.int32)
        N.check(N.lib().bb_get_terrain_rng(self._h, None if w is None else w.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           s.ctypes.data_as(C.POINTER(C.c_int32))), "bb_get_terrain_rng")
        return w, s

    def get_attr(self, name: str, indices=None):
        n = self.num_envs if indices is None else len(list(indices))
        return [getattr(self, name)] * n

    def set_attr(self, name: str, value, indices=None) -> None:
        setattr(self, name, value)

    def env_method(self, name: str, *args, indices=None, **kwargs):
        n = self.num_envs if indices is None else len(list(indices))
        return [getattr(self, name)(*args, **kwargs)] * n

    def env_is_wrapped(self, wrapper_class, indices=None):
        n = self.num_envs if indices is None else len(list(indices))
        return [False] * n

    def obs_dict(self, obs: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        o = self.obs if obs is None else obs
        d = {k: o[:, 3 * i:3 * i + 3] for i, k in enumerate(OBS_KEYS)}
        if self.cameras:  # the reference's camera keys (ballbot_env.py:812-826), channels-first
            if self.cam_channels == 4:
                d["rgbd_0"], d["rgbd_1"] = self.rgbd[:, 0], self.rgbd[:, 1]
            else:
                d["rgbd_0"] = self.depth[:, 0:1]
                d["rgbd_1"] = self.depth[:, 1:2]
            d["relative_image_timestamp"] = self.rel_ts.unsqueeze(1)
        return dict(sorted(d.items()))

    # ------------------------------------------------------------ parity/state
    def get_state(self):
        n = self.num_envs
        q, v, w = np.zeros((n, N.NQ)), np.zeros((n, N.NV)), np.zeros((n, N.NV))
        s = np.zeros(n, dtype=np.int32)
        dp = C.POINTER(C.c_double)
        N.check(N.lib().bb_get_state(self._h, q.ctypes.data_as(dp), v.ctypes.data_as(dp), w.ctypes.data_as(dp),
                                     s.ctypes.data_as(C.POINTER(C.c_int32))), "bb_get_state")
        return q, v, w, s

    def set_state(self, qpos, qvel, warm=None, steps=None):
        n = self.num_envs
        q = np.ascontiguousarray(np.broadcast_to(qpos, (n, N.NQ)), dtype=np.float64)
        v = np.ascontiguousarray(np.broadcast_to(qvel, (n, N.NV)), dtype=np.float64)
        w = np.zeros((n, N.NV)) if warm is None else np.ascontiguousarray(np.broadcast_to(warm, (n, N.NV)),
                                                                           dtype=np.float64)
        s = np.zeros(n, np.int32) if steps is None else np.ascontiguousarray(np.broadcast_to(steps, (n,)),
                                                                              dtype=np.int32)
        dp = C.POINTER(C.c_double)
        N.check(N.lib().bb_set_state(self._h, q.ctypes.data_as(dp), v.ctypes.data_as(dp), w.ctypes.data_as(dp),
                                     s.ctypes.data_as(C.POINTER(C.c_int32))), "bb_set_state")

    def forward(self, ctrl):
        """mj_forward at the current state (diagnostic): returns qacc [N,15] and contact
        counts [N,2] = (ball-hfield, base-tree geoms)."""
        n = self.num_envs
        c = np.ascontiguousarray(np.broadcast_to(ctrl, (n, 3)), dtype=np.float64)
        qacc = np.zeros((n, N.NV))
        ncon = np.zeros((n, 2), np.int32)
        dp = C.POINTER(C.c_double)
        N.check(N.lib().bb_forward(self._h, c.ctypes.data_as(dp), qacc.ctypes.data_as(dp),
                                   ncon.ctypes.data_as(C.POINTER(C.c_int32))), "bb_forward")
        return qacc, ncon

    def stats(self) -> Dict[str, int]:
        out = (C.c_int64 * N.NSTATS)()
        N.check(N.lib().bb_get_stats(self._h, out, N.NSTATS), "bb_get_stats")
        return {"resets": out[0], "diverged": out[1], "overflow": out[2], "slow_path": out[3],
                "solver_iters": out[4], "stream_wraps": out[5], "spill": out[6], "pair_budget": out[7]}

    def pair_counters(self) -> Dict[str, int]:
        """Diagnostics of the last relief-pair launch of step_multi (bb_pair_counters; waits for the device)."""
        keys = ("busy_fast", "busy_full", "idle_fast", "idle_full", "active_fast", "active_full", "claims_fast",
                "claims_full", "steps_fast", "steps_full", "handovers", "life_cycles_fast", "life_cycles_full",
                "life_wall_fast", "life_wall_full", "heavy", "ring_len", "ring_pushes_min_fast", "ring_pushes_min_full")
        out = (C.c_int64 * len(keys))()
        N.check(N.lib().bb_pair_counters(self._h, out, len(keys)), "bb_pair_counters")
        return dict(zip(keys, out))

    def pair_env_times(self):
        """Per env, the last relief-pair launch: (shader cycles its steps took, wall tick of its last step)."""
        out = np.zeros((2, self.num_envs), np.uint64)
        N.check(N.lib().bb_pair_env_times(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))), "bb_pair_env_times")
        return out[0], out[1]

    def env_terrain(self):
        """(bank slot of every env's current terrain, stream draws each env made) as int32[N] arrays."""
        t = np.zeros(self.num_envs, np.int32)
        k = np.zeros(self.num_envs, np.int32)
        ip = C.POINTER(C.c_int32)
        N.check(N.lib().bb_get_env_terrain(self._h, t.ctypes.data_as(ip), k.ctypes.data_as(ip)), "bb_get_env_terrain")
        return t, k

    def assign_terrain(self, ids) -> None:
        """Pin env i to bank slot ids[i] for its later resets (-1 unpins: back to its stream)."""
        t = torch.as_tensor(np.asarray(ids, np.int32)).to(self.device)
        N.check(N.lib().bb_assign_terrain(self._h, _ptr(t), self._stream()), "bb_assign_terrain")
        torch.cuda.current_stream(self.device).synchronize()

    def hfield(self, terrain_id: int) -> np.ndarray:
        """Terrain bank slot `terrain_id` as float32[293*293] (host copy)."""
        out = np.empty(N.HF_N * N.HF_N, np.float32)
        N.check(N.lib().bb_get_hfield(self._h, int(terrain_id), out.ctypes.data_as(C.POINTER(C.c_float))),
                "bb_get_hfield")
        return out

    def time_kernel(self, max_launches: int) -> None:
        """Time the next `max_launches` fast step kernels with HIP events (bench.py)."""
        N.check(N.lib().bb_time_kernel(self._h, int(max_launches)), "bb_time_kernel")

    def kernel_ms(self):
        """(average fast-step-kernel duration in ms, launches timed) since time_kernel()."""
        ms, k = C.c_double(), C.c_int32()
        N.check(N.lib().bb_kernel_ms(self._h, C.byref(ms), C.byref(k)), "bb_kernel_ms")
        return ms.value, k.value

    def kernel_times(self):
        """Average ms of the fast kernel, the predicted full kernel (route 0, side stream) and
        the hand-over full kernel over the steps timed since time_kernel(); and the count."""
        t, k = (C.c_double * 3)(), C.c_int32()
        N.check(N.lib().bb_kernel_times(self._h, t, C.byref(k)), "bb_kernel_times")
        return {"fast": t[0], "predicted_full": t[1], "handover_full": t[2]}, k.value

    def launch_config(self) -> Dict[str, int]:
        out = (C.c_int32 * 5)()
        N.check(N.lib().bb_get_config(self._h, out), "bb_get_config")
        return {"num_envs": out[0], "envs_per_wave": out[1], "fp64": out[2], "lds_bytes_per_workgroup": out[3],
                "lanes_per_env": out[4]}

    def offsets(self) -> np.ndarray:
        o = np.zeros(self.n_terrains, np.float32)
        N.check(N.lib().bb_get_offsets(self._h, o.ctypes.data_as(C.POINTER(C.c_float))), "bb_get_offsets")
        return o

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_log_on", False):
                self.flush_logs()
            N.lib().bb_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def split_obs(obs15) -> Dict[str, Any]:
    return {k: obs15[3 * i:3 * i + 3] for i, k in enumerate(OBS_KEYS)}
