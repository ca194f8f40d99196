"""What the shadow audit costs while it is on (kz_engine_set_audit): the decoded host-boundary rate of chess
20 x 256 f16 at batch 256 through capi on four slots — submit on a slot, wait for the oldest — with the audit off and with
(period, boards, dtype) = (16, 16, split16), (16, 16, f32) and (1, 16, split16), in interleaved rounds inside one process; each
setting's median rate and its fraction of the off rate.  The sampled boards run on the sibling engine's own stream beside the
batch, and the returning call waits for them, so the cost is the sibling's launch sharing the chip plus whatever of it the batch
does not hide.  Prints one JSON object; --out writes it to a file as well.

    python tools/audit_cost.py [--rounds 5] [--batches 200] [--depth 20] [--channels 256] [--out profiles/x.json]
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

SETTINGS = (("off", None), ("16:16:split16", (capi.KZ_DTYPE_F32_SPLIT16, 16, 16)), ("16:16:f32", (capi.KZ_DTYPE_F32, 16, 16)),
            ("1:16:split16", (capi.KZ_DTYPE_F32_SPLIT16, 1, 16)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=200, help="batches per timed run")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert capi.device_count() >= 1, "needs a GPU"

    eng = capi.Engine(capi.Model(blob=synth.random_model("chess", args.depth, args.channels, "attention", seed=3)), 0, args.batch,
                      capi.KZ_DTYPE_F16)
    policy_len = eng.model.info.policy_len
    rng = np.random.default_rng(1)
    bits, scalars = synth.random_boards("chess", args.batch, seed=2)
    moves = [rng.permutation(policy_len)[:int(n)].astype(np.int32) for n in rng.integers(1, 61, size=args.batch)]
    offsets, idx = eng._csr(moves)
    slots = capi.KZ_ENGINE_SLOTS

    def run(n):
        """n batches through the four slots, the oldest waited for before its slot is submitted on again: evals/s."""
        t0 = time.perf_counter()
        for i in range(n):
            if i >= slots:
                eng.wait_decoded_view(i % slots)
            eng.submit_packed_decoded_csr(i % slots, bits, scalars, offsets, idx)
        for i in range(max(n - slots, 0), n):
            eng.wait_decoded_view(i % slots)
        return n * args.batch / (time.perf_counter() - t0)

    def setting(audit):
        if audit is None:
            eng.set_audit(-1, 0, 0)
        else:
            eng.set_audit(*audit)

    rates = {name: [] for name, _ in SETTINGS}
    audited = {}
    for name, audit in SETTINGS:  # warm-up: each sibling's creation and first launch, the staging's first growth
        setting(audit)
        run(2 * slots + (audit[1] if audit else 0))
    for _ in range(args.rounds):
        for name, audit in SETTINGS:
            setting(audit)
            rates[name].append(run(args.batches))
            if audit:
                audited[name] = eng.audit_stats().batches
    med = {name: statistics.median(v) for name, v in rates.items()}
    out = {"tool": "audit_cost", "tower_path": eng.tower_path, "batch": args.batch, "rounds": args.rounds, "batches_per_run": args.batches,
           "network": f"chess {args.depth}x{args.channels} f16", "slots": slots,
           "evals_per_s_median": {name: round(med[name]) for name in med},
           "evals_per_s_min_max": {name: [round(min(v)), round(max(v))] for name, v in rates.items()},
           "fraction_of_off": {name: round(med[name] / med["off"], 4) for name in med if name != "off"},
           "audited_batches_per_run": audited}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
