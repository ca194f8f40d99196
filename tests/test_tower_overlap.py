"""The chess f16 one-launch tower (kz_tower.hip) against its previous instance, kept in the experiment build only
(experiments/libkzhip_exp.so, KZ_TOWER_PREV=1): the k-loop's weight addresses and tap rows are computed differently, the
arithmetic is not touched, so every output must be BIT-identical — raw scalars and policy rows, and the decoded values
and move probabilities.  Run in a child process with KZ_LIB_PATH set, so that this process keeps the product library."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP_LIB = os.path.join(REPO, "experiments", "libkzhip_exp.so")

# (game, depth, channels, head, batches)
CASES = [
    ("chess", 20, 256, "attention", (256, 37)),  # the flagship network; 37: a partial last workgroup
    ("chess-hist-2", 2, 256, "attention", (64, 9)),  # 47 input planes: the WIDE stem
    ("chess", 2, 256, "dense", (64, 5)),  # no attention heads: the tower-only launch
]


def _engines(model, capi, batch):
    os.environ["KZ_TOWER_PREV"] = "1"
    try:
        prev = capi.Engine(model, 0, batch, capi.KZ_DTYPE_F16)
    finally:
        del os.environ["KZ_TOWER_PREV"]
    cur = capi.Engine(model, 0, batch, capi.KZ_DTYPE_F16)
    return prev, cur


def _child():
    from kzero_amd import capi, synth
    assert capi.LIB_PATH.endswith("libkzhip_exp.so")
    for game, depth, channels, head, batches in CASES:
        blob = synth.random_model(game, depth, channels, head, seed=41)
        model = capi.Model(blob=blob)
        prev, cur = _engines(model, capi, max(batches))
        assert prev.tower_path == cur.tower_path and cur.tower_path.startswith("tower_resident_f16"), cur.tower_path
        for n in batches:
            bits, scalars_in = synth.random_boards(game, n, seed=42 + n)
            s0, p0 = prev.eval_packed(bits, scalars_in)
            s1, p1 = cur.eval_packed(bits, scalars_in)
            assert np.array_equal(s0, s1), f"{game} {depth}x{channels} {head} batch {n}: scalars differ"
            assert np.array_equal(p0, p1), f"{game} {depth}x{channels} {head} batch {n}: policy differs"
            if cur.tower_path.endswith("+heads"):  # decode_output inside the launch
                rng = np.random.default_rng(n)
                moves = [rng.permutation(p0.shape[1])[:int(k)].astype(np.int32) for k in rng.integers(0, 60, n)]
                v0, q0 = prev.eval_packed_decoded(bits, scalars_in, moves)
                v1, q1 = cur.eval_packed_decoded(bits, scalars_in, moves)
                assert np.array_equal(v0, v1), f"{game} batch {n}: decoded values differ"
                assert all(np.array_equal(a, b) for a, b in zip(q0, q1)), f"{game} batch {n}: probabilities differ"
            print(f"{game} {depth}x{channels} {head} [{cur.tower_path}] batch {n}: identical")


@pytest.mark.gpu
def test_tower_is_bit_identical_to_its_previous_instance():
    if not os.path.exists(EXP_LIB):  # (the experiment library is built best effort: __graft_entry__.build())
        pytest.skip("libkzhip_exp.so is not built: experiments/build.sh")
    env = dict(os.environ, KZ_LIB_PATH=EXP_LIB)
    r = subprocess.run([sys.executable, "-c", "from tests import test_tower_overlap as t; t._child()"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=900)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-30:])
    assert r.returncode == 0, tail
    print(tail)
