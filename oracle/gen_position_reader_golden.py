#!/usr/bin/env python3
"""Writes tests/golden/position_reader.npz: what the reference's own reader of the position record format
(python/lib/data/file.py + position.py) reads from two files this repository writes — the Python writer's Ataxx file and
the C++ writer's chess file of tests/test_position_file.py — together with the SHA-256 of the bytes it read.  Data, not
source: the tests check that the writers still produce those exact bytes and hold the recorded reading to the records,
on any box, without the reference present.

    python oracle/gen_position_reader_golden.py <reference>/python
"""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "position_reader.npz")
sys.path.insert(0, REPO)


def record(case, path, game, DataFile, Game):
    df = DataFile.open(Game.find(game), path)
    pos = [df.positions[i] for i in range(len(df.positions))]
    sims = [df.simulations[i] for i in range(len(df.simulations))]
    counts = np.array([p.available_mv_count for p in pos], np.int64)
    return {
        f"{case}_sha256": np.array([hashlib.sha256(open(path + ext, "rb").read()).hexdigest() for ext in (".bin", ".off", ".json")]),
        f"{case}_move_index": np.array([p.move_index for p in pos], np.int64),
        f"{case}_available_mv_count": counts,
        f"{case}_input_bools": np.stack([np.asarray(p.input_bools, np.uint8) for p in pos]),
        f"{case}_input_scalars": np.stack([np.asarray(p.input_scalars, np.float32) for p in pos]),
        f"{case}_policy_offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
        f"{case}_policy_indices": np.concatenate([np.asarray(p.policy_indices, np.int32) for p in pos]),
        f"{case}_policy_values": np.concatenate([np.asarray(p.policy_values, np.float32) for p in pos]),
        f"{case}_zero_v": np.array([p.zero_v for p in pos], np.float64),
        f"{case}_is_final": np.array([p.is_final for p in pos], bool),
        f"{case}_sim_start_file_pi": np.array([s.start_file_pi for s in sims], np.int64),
        f"{case}_sim_move_count": np.array([s.move_count for s in sims], np.int64),
    }


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.dont_write_bytecode = True
    sys.path.insert(0, sys.argv[1])
    from lib.data.file import DataFile
    from lib.games import Game
    from tests.test_position_file import _games, _tool, _write
    out = {}
    with tempfile.TemporaryDirectory() as d:
        # the file of test_reference_reader_accepts_our_files
        path = os.path.join(d, "games_7")
        games, shape, ns, pshape = _games(np.random.default_rng(2))
        _write(path, games, shape, ns, pshape)
        out.update(record("ours", path, "ataxx-7", DataFile, Game))
        # the file of test_reference_reader_accepts_the_cpp_writers_files
        path = os.path.join(d, "games_9")
        subprocess.run([_tool(), "write", path, "5", "4"], capture_output=True, text=True, check=True)
        out.update(record("cpp", path, "chess", DataFile, Game))
    np.savez_compressed(OUT, **out)
    print(f"{len(out)} arrays -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
