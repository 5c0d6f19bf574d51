"""bb_eval_track's accounting without a GPU: csrc/bb_eval.h compiled for the host
(tests/hostcheck/eval_track_check.cpp) against the numpy restatement of evaluate_policy's loop
(tests/eval_track_ref.py) on random reward / flag streams.  Everything is exact: the only arithmetic
is a float64 sum of float32 rewards in step order, which both sides do in the same order."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import eval_track_ref as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openballbot-rl_amd" / "csrc"
INCLUDE = ROOT / "include"
SRC = ROOT / "tests" / "hostcheck" / "eval_track_check.cpp"
LIB = ROOT / "tests" / "_build" / "libeval_track_check.so"

FIELDS = ("reward", "flags", "obs", "rel_ts", "targets", "ep_ret", "ep_len", "counts", "tab_ret", "tab_len",
          "tab_env", "tab_step", "book", "feats", "fresh")


class Args(C.Structure):
    _fields_ = [("n", C.c_int32), ("cap", C.c_int32)] + [(k, C.c_void_p) for k in FIELDS]


@pytest.fixture(scope="module")
def host():
    LIB.parent.mkdir(parents=True, exist_ok=True)
    srcs = [SRC, CSRC / "bb_eval.h", INCLUDE / "ballbot_mi355x.h"]
    if not LIB.exists() or any(LIB.stat().st_mtime < s.stat().st_mtime for s in srcs):
        subprocess.run(["hipcc", "-x", "c++", "-O2", "-std=c++17", "-fPIC", "-shared", f"-I{CSRC}", f"-I{INCLUDE}",
                        "-o", str(LIB), str(SRC)], check=True, capture_output=True)
    L = C.CDLL(str(LIB))
    L.ec_eval_track.argtypes = [C.POINTER(Args)]
    L.ec_eval_track.restype = C.c_int
    return L


def _p(a):
    return None if a is None else a.ctypes.data


class HostState:
    """The arrays one bb_eval_track caller owns, as the kernel tests lay them out."""

    def __init__(self, n, targets, cap):
        ref = R.TrackRef(n, targets, cap)  # the same initial values, sentinels included
        self.n, self.cap = n, cap
        for k in ("targets", "ep_ret", "ep_len", "counts", "tab_ret", "tab_len", "tab_env", "tab_step", "book"):
            setattr(self, k, getattr(ref, k).copy())
        self.feats = np.full((n, 56), R.SENTINEL, np.float32)
        self.fresh = np.full(n, -5, np.int64)

    def args(self, reward, flags, obs, rel_ts, stage=True):
        return Args(self.n, self.cap, _p(reward), _p(flags), _p(obs), _p(rel_ts), _p(self.targets), _p(self.ep_ret),
                    _p(self.ep_len), _p(self.counts), _p(self.tab_ret), _p(self.tab_len), _p(self.tab_env),
                    _p(self.tab_step), _p(self.book), _p(self.feats) if stage else None,
                    _p(self.fresh) if stage else None)


def assert_state_equal(got, ref):
    for k in ("ep_ret", "ep_len", "counts", "tab_ret", "tab_len", "tab_env", "tab_step", "book"):
        np.testing.assert_array_equal(getattr(got, k), getattr(ref, k), err_msg=k)


# (n, E): E < n (some envs owe nothing), E = n, E = n + 2 (two envs owe two); n = 1 has no E in [1, n)
CASES = [(n, E) for n in (1, 63, 64, 65, 1025) for E in (n // 2, n, n + 2) if E >= 1]


@pytest.mark.parametrize("n,E", CASES)
def test_accounting_equals_the_numpy_restatement(host, n, E):
    """p(done) = 0.2 over 50 steps; targets (E + i) // n with E < n, E = n and E = n + 2."""
    reward, flags, obs, rel_ts = R.streams(n)
    tg = R.targets_for(E, n)
    assert tg.sum() == E
    ref, got = R.TrackRef(n, tg, E), HostState(n, tg, E)
    feats_ref, fresh_ref = got.feats.copy(), got.fresh.copy()
    multi = 0
    for t in range(reward.shape[0]):
        before = int(ref.book[0])
        ref.step(reward[t], flags[t])
        multi += int(ref.book[0]) - before >= 2
        R.stage_ref(obs[t], rel_ts[t], feats_ref, fresh_ref)
        a = got.args(reward[t], flags[t], obs[t], rel_ts[t])
        assert host.ec_eval_track(C.byref(a)) == 0
        assert_state_equal(got, ref)
        np.testing.assert_array_equal(got.feats, feats_ref)
        np.testing.assert_array_equal(got.fresh, fresh_ref)
    listed = int(ref.book[0])
    assert listed >= 1 and listed + ref.book[1] == E and ref.book[3] == 0 and ref.book[2] == reward.shape[0]
    assert (got.feats[:, 13:53] == R.SENTINEL).all()
    assert n < 3 or multi > 0, "no step listed two episodes: the case does not test the order"
    assert (ref.counts <= tg).all() and ref.counts.sum() == listed and (np.diff(ref.tab_step[:listed]) >= 0).all()
    assert (got.tab_ret[listed:] == R.SENTINEL).all() and (got.tab_env[listed:] == -7).all()


def test_table_overflow_sets_the_flag_and_writes_nothing_past_cap(host):
    n, E, cap = 65, 67, 40
    reward, flags, _, _ = R.streams(n, seed=2)
    tg = R.targets_for(E, n)
    ref, got = R.TrackRef(n, tg, cap), HostState(n, tg, cap)
    # the arrays hold 8 more rows than cap says: they must keep their sentinels
    for s in (ref, got):
        s.tab_ret = np.full(cap + 8, R.SENTINEL, np.float64)
        s.tab_len, s.tab_step = np.full(cap + 8, -7, np.int64), np.full(cap + 8, -7, np.int64)
        s.tab_env = np.full(cap + 8, -7, np.int32)
    for t in range(reward.shape[0]):
        ref.step(reward[t], flags[t])
        assert host.ec_eval_track(C.byref(got.args(reward[t], flags[t], None, None, stage=False))) == 0
        assert_state_equal(got, ref)
    assert got.book[3] == 1 and got.book[0] == E and got.book[1] == 0
    assert (got.tab_ret[cap:] == R.SENTINEL).all() and (got.tab_env[cap:] == -7).all()
    assert (got.tab_env[:cap] >= 0).all()


def test_priming_call_only_stages(host):
    n = 65
    _, _, obs, rel_ts = R.streams(n, seed=3)
    got = HostState(n, R.targets_for(8, n), 8)
    before = {k: getattr(got, k).copy() for k in ("ep_ret", "ep_len", "counts", "tab_ret", "book")}
    ts = np.zeros(n, np.float32)  # after a reset every camera has just rendered
    assert host.ec_eval_track(C.byref(got.args(None, None, obs[0], ts))) == 0
    for k, v in before.items():
        np.testing.assert_array_equal(getattr(got, k), v)
    np.testing.assert_array_equal(got.fresh, np.arange(n))
    np.testing.assert_array_equal(got.feats[:, 0:12], obs[0][:, 0:12])
    assert (got.feats[:, 12] == 0).all() and (got.feats[:, 13:53] == R.SENTINEL).all()
    # without cameras: column 12 keeps its value, nothing is fresh
    got.feats[:, 12] = 5.0
    assert host.ec_eval_track(C.byref(got.args(None, None, obs[1], None))) == 0
    assert (got.fresh == -1).all() and (got.feats[:, 12] == 5.0).all()
    np.testing.assert_array_equal(got.feats[:, 53:56], obs[1][:, 12:15])
