"""Measures the averaged-symmetry entry (kz_engine_submit_packed_decoded_avg) on one GPU, in one process,
in interleaved rounds:

  A  the averaged entry at batch max_batch / n_sym  (each board and move list crosses PCIe once, the device fans out and averages)
  B  the `_sym` entry at batch max_batch fed the replicated boards and ids 0 .. n_sym-1  (the same network work; what a caller
     without the entry would submit — without the host-side averaging it would still have to do)

both with all four slots in flight from one thread, then the kz_engine_kernel_time of the two new kernels in a profiled pass
of its own.  Prints one JSON object; --out writes it to a file as well.

    python tools/symmetry_average_bench.py [--rounds 7] [--batches 2000] [--out profiles/x.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from kzero_amd import capi, synth  # noqa: E402
from tests.test_gpu_symmetry import ataxx_tables, move_lists  # noqa: E402

SLOTS = capi.KZ_ENGINE_SLOTS


def pipelined(eng, submit, batches):
    """`batches` submissions with every slot in flight; seconds from the first submit to the last wait."""
    t0 = time.perf_counter()
    for s in range(SLOTS):
        submit(s)
    for i in range(batches):
        s = i % SLOTS
        eng.wait_decoded_view(s)
        if i + SLOTS < batches:
            submit(s)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=2000, help="batches per round and entry")
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert capi.device_count() >= 1, "needs a GPU"

    square_src, policy_map = ataxx_tables(7)
    n_sym = len(square_src)
    eng = capi.Engine(capi.Model(blob=synth.random_model("ataxx-7", args.depth, args.channels, "ataxx_conv", seed=5)), 0, args.max_batch,
                      capi.KZ_DTYPE_F16)
    eng.set_symmetries(square_src, policy_map)
    batch = args.max_batch // n_sym
    rng = np.random.default_rng(1)
    valid = np.flatnonzero((policy_map >= 0).all(axis=0))
    bits, scalars = synth.random_boards("ataxx-7", batch, seed=2)
    moves = move_lists(rng, valid, batch, finished=3)
    off, idx = eng._csr(moves)
    r_bits, r_scalars = np.ascontiguousarray(np.repeat(bits, n_sym, axis=0)), np.ascontiguousarray(np.repeat(scalars, n_sym, axis=0))
    r_off, r_idx = eng._csr([m for m in moves for _ in range(n_sym)])
    ids = np.tile(np.arange(n_sym), batch).astype(np.uint8)

    def submit_avg(slot):
        eng.submit_packed_decoded_avg_csr(slot, bits, scalars, off, idx)

    def submit_sym(slot):
        eng.submit_packed_decoded_csr(slot, r_bits, r_scalars, r_off, r_idx, sym=ids)

    for submit in (submit_avg, submit_sym):  # warm-up: code objects, scratch, staging
        pipelined(eng, submit, 200)
    rates = {"avg": [], "sym": []}
    for _ in range(args.rounds):
        for name, submit in (("avg", submit_avg), ("sym", submit_sym)):
            rates[name].append(args.batches * batch * n_sym / pipelined(eng, submit, args.batches))

    eng.set_profiling(True)  # a pass of its own: the events slow the host
    profiled = 400
    pipelined(eng, submit_avg, profiled)
    kernels = {}
    for k in ("kz_sym_fan_out", "kz_sym_average", "kz_tower", "kz_decode_output"):
        ms, n = eng.kernel_time(k)
        kernels[k] = {"launches": n, "mean_us": 1e3 * ms / n if n else None}
    eng.set_profiling(False)

    def stats(x):
        return {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x)), "runs": [float(v) for v in x]}

    result = {
        "what": "averaged-symmetry entry against the _sym entry on the replicated batch, network evaluations (virtual boards) per second",
        "network": f"ataxx-7 {args.depth}x{args.channels} ataxx_conv f16", "tower_path": eng.tower_path, "max_batch": args.max_batch, "n_sym": n_sym,
        "avg_entry_batch": batch, "sym_entry_batch": batch * n_sym, "slots_in_flight": SLOTS, "rounds": args.rounds, "batches_per_round": args.batches,
        "moves_per_batch": int(off[-1]),
        "avg_entry_network_evals_per_s": stats(rates["avg"]), "sym_entry_network_evals_per_s": stats(rates["sym"]),
        "avg_entry_positions_per_s": float(np.median(rates["avg"])) / n_sym,
        "kernel_time_profiled_pass": kernels,
    }
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
