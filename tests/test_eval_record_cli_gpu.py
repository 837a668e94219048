"""train/evaluate_native.py with the recording options, once, in a child process: the pickle has rollout.py's structure
(train/rllib/rollout.py:20-28), the frames file one array per episode, and the printed episode rewards are the sums of the pickle."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

from gpu_support import ROOT, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


def test_script_records_two_envs(torch_cuda, tmp_path):
    F, G = str(tmp_path / "rollouts.pkl"), str(tmp_path / "frames.npz")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train", "evaluate_native.py"), "--envs", "256", "--episodes", "1",
                          "--record-envs", "0,255", "--out", F, "--frames", G, "--frame-size", "24x16"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert lines[0].split()[:2] == ["policy", "episodes"] and int(lines[1].split()[1]) == 256   # the table is what it was
    assert not any(l.startswith("warning") for l in lines)                               # the default capacity always suffices
    with open(F, "rb") as f:
        rollouts = pickle.load(f)
    assert isinstance(rollouts, list) and len(rollouts) == 2                             # one episode per env, two envs
    for ep in rollouts:
        assert isinstance(ep, list) and 1 <= len(ep) <= 1000
        for state, action, next_state, reward, done in ep:
            assert state.dtype == np.float64 and state.shape == next_state.shape and state.ndim == 1
            assert isinstance(action, int) and 0 <= action < 3 and isinstance(reward, float) and isinstance(done, bool)
        assert [step[4] for step in ep] == [False] * (len(ep) - 1) + [True]
        assert all(np.array_equal(a[2], b[0]) for a, b in zip(ep, ep[1:]))               # next_state is the next step's state
    frames = np.load(G)
    assert sorted(frames.files) == ["episode_0000", "episode_0001"]
    for i, ep in enumerate(rollouts):
        a = frames["episode_%04d" % i]
        assert a.dtype == np.uint8 and a.shape == (len(ep), 16, 24, 3)
        assert ((a == (0, 0, 200)).all(axis=-1) | (a == (139, 69, 19)).all(axis=-1)).any(axis=(1, 2)).all()   # water or bank in every frame
    printed = [float(re.match(r"Episode reward (\S+)", l).group(1)) for l in lines if l.startswith("Episode reward")]
    sums = []
    for ep in rollouts:
        total = 0.0
        for step in ep:
            total += step[3]
        sums.append(total)
    assert printed == sums
