"""What a fell-back board costs (kz_engine_set_range_fallback): the time one thread spends from
kz_engine_submit_packed_decoded to the return of kz_engine_wait_decoded_status for a chess 20 x 256 f16 batch of 256 with 0, 1, 3
and 16 boards out of the f16 range (scalars_in[b, 0] = 3e5), one batch in flight, in interleaved rounds; the median per count and
its difference to the count 0.  The flagged boards are re-evaluated by the exact-f32 sibling engine inside the wait, so the
difference is a synchronous exact-f32 launch of that many boards plus the gather and the patch on the host.
Prints one JSON object; --out writes it to a file as well.

    python tools/range_fallback_cost.py [--rounds 30] [--depth 20] [--channels 256] [--out profiles/x.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from kzero_amd import capi, synth  # noqa: E402

COUNTS = (0, 1, 3, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert capi.device_count() >= 1, "needs a GPU"

    eng = capi.Engine(capi.Model(blob=synth.random_model("chess", args.depth, args.channels, "attention", seed=3)), 0, args.batch,
                      capi.KZ_DTYPE_F16)
    eng.set_range_fallback(capi.KZ_DTYPE_F32)
    policy_len = eng.model.info.policy_len
    rng = np.random.default_rng(1)
    bits, scalars = synth.random_boards("chess", args.batch, seed=2)
    moves = [rng.permutation(policy_len)[:int(n)].astype(np.int32) for n in rng.integers(1, 61, size=args.batch)]
    offsets, idx = eng._csr(moves)
    inputs = {}
    for k in COUNTS:
        s = scalars.copy()
        s[rng.permutation(args.batch)[:k], 0] = 3e5
        inputs[k] = np.ascontiguousarray(s)

    def once(k):
        t0 = time.perf_counter()
        eng.submit_packed_decoded_csr(0, bits, inputs[k], offsets, idx)
        _, _, status = eng.wait_decoded_status(0, offsets)
        dt = time.perf_counter() - t0
        assert int((status == capi.KZ_BOARD_FELL_BACK).sum()) == k and int((status != 0).sum()) == k, status
        return dt * 1e3

    for k in COUNTS:  # warm-up: the sibling's first launch, the staging's first growth
        once(k)
    times = {k: [] for k in COUNTS}
    for _ in range(args.rounds):
        for k in COUNTS:
            times[k].append(once(k))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"tool": "range_fallback_cost", "tower_path": eng.tower_path, "batch": args.batch, "rounds": args.rounds,
           "network": f"chess {args.depth}x{args.channels} f16",
           "submit_to_wait_ms_median": {str(k): round(med[k], 4) for k in COUNTS},
           "submit_to_wait_ms_min_max": {str(k): [round(min(times[k]), 4), round(max(times[k]), 4)] for k in COUNTS},
           "added_ms_median": {str(k): round(med[k] - med[0], 4) for k in COUNTS if k}}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
