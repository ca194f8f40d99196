#!/usr/bin/env python3
"""KZ_DTYPE_BF16 against KZ_DTYPE_F16 on the same network (bench.py measures the flagship in its own dtypes and stays as it is):
the decoded host-boundary rate — submit_packed_decoded on the four slots, the oldest waited for before its slot is used again —
of both engines in ONE process, in interleaved timed regions (kzero_amd.benchlib.run_timed: device sync on both sides of every
region), the median of 7 regions each.  Networks and batches: README's rows — chess 20x256 at 256, Ataxx 7x7 8x128 at 256, Go 9x9
16x128 at 2048.

--contract adds what the bf16 arithmetic costs in precision on chess 20x256 at batch 256 against the CPU oracle
(tests/oracle_lib.py): max |delta| / scale and rms / scale per board and output tensor, and the post-softmax max |delta p| over
the whole policy, with the f16 engine's figures on the same boards beside them.  Prints one JSON object; --out writes it too.

    python tools/bf16_rate.py [--regions 7] [--seconds 0.5] [--nets chess,ataxx,go9] [--contract] [--out profiles/x.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from kzero_amd import benchlib, capi, synth  # noqa: E402

NETS = {"chess": ("chess", 20, 256, "attention", 256), "ataxx": ("ataxx-7", 8, 128, "ataxx_conv", 256),
        "go9": ("go-9", 16, 128, "conv", 2048)}
DTYPES = (("bf16", capi.KZ_DTYPE_BF16), ("f16", capi.KZ_DTYPE_F16))


class Loop:
    """One engine's four-slot loop as benchlib's (step, sync) pair."""

    def __init__(self, eng, bits, scalars, offsets, idx):
        self.eng, self.args, self.busy = eng, (bits, scalars, offsets, idx), [False] * capi.KZ_ENGINE_SLOTS

    def step(self, i):
        slot = i % len(self.busy)
        if self.busy[slot]:
            self.eng.wait_decoded_view(slot)
        self.eng.submit_packed_decoded_csr(slot, *self.args)
        self.busy[slot] = True

    def sync(self):
        for slot, busy in enumerate(self.busy):
            if busy:
                self.eng.wait_decoded_view(slot)
                self.busy[slot] = False


def rates(key, regions, seconds):
    game, depth, channels, head, batch = NETS[key]
    model = capi.Model(blob=synth.random_model(game, depth, channels, head, seed=3))
    rng = np.random.default_rng(1)
    bits, scalars = synth.random_boards(game, batch, seed=2)
    moves = [rng.permutation(model.info.policy_len)[:int(n)].astype(np.int32) for n in rng.integers(1, 61, size=batch)]
    loops, paths = {}, {}
    for name, dtype in DTYPES:
        eng = capi.Engine(model, 0, batch, dtype)
        offsets, idx = eng._csr(moves)
        loops[name], paths[name] = Loop(eng, bits, scalars, offsets, idx), eng.tower_path
    # steps per region from a first look at the slower engine: about `seconds` per region, at least four rounds of the slots
    steps = {}
    for name, loop in loops.items():
        t = benchlib.run_timed(loop.step, loop.sync, 8, 8)
        steps[name] = max(16, int(seconds / (t / 8)))
    elapsed = {name: [] for name in loops}
    for _ in range(regions):  # interleaved: both engines see the same minutes of the chip
        for name, loop in loops.items():
            elapsed[name].append(benchlib.run_timed(loop.step, loop.sync, steps[name], 4))
    out = {"network": f"{game} {depth}x{channels}", "batch": batch, "regions": regions}
    for name in loops:
        med = benchlib.median_region(elapsed[name])
        out[name] = {"tower_path": paths[name], "steps_per_region": steps[name], "evals_per_s_median": round(steps[name] * batch / med),
                     "evals_per_s_min_max": [round(steps[name] * batch / max(elapsed[name])), round(steps[name] * batch / min(elapsed[name]))]}
    out["bf16_over_f16"] = round(out["bf16"]["evals_per_s_median"] / out["f16"]["evals_per_s_median"], 3)
    return out


def contract(batch=256):
    from tests import oracle_lib as O
    blob = synth.random_model("chess", 20, 256, "attention", seed=3)
    bits, scalars = synth.random_boards("chess", batch, seed=2)
    net = O.OracleNet(blob)
    s_ref, p_ref = net.forward(O.encode_input_full(bits, scalars, net.n_scalar, net.n_bool, net.h, net.w), threads=min(16, os.cpu_count() or 1))

    def softmax(x):
        e = np.exp(x - x.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)

    out = {"network": "chess 20x256", "batch": batch, "reference": "CPU oracle (f32)",
           "scale": {"scalars": float(np.abs(s_ref).max()), "policy": float(np.abs(p_ref).max())}}
    model = capi.Model(blob=blob)
    for name, dtype in DTYPES:
        s, p = capi.Engine(model, 0, batch, dtype).eval_packed(bits, scalars)
        row = {}
        for what, a, ref in (("scalars", s, s_ref), ("policy", p, p_ref)):
            d = (a.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref).max(axis=-1, keepdims=True))
            row[what] = {"max_over_scale": float(np.abs(d).max()), "rms_over_scale": float(np.sqrt(np.mean(d ** 2)))}
        row["softmax_max_abs_dp"] = float(np.abs(softmax(p.astype(np.float64)) - softmax(p_ref.astype(np.float64))).max())
        out[name] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.5, help="length of a timed region")
    ap.add_argument("--nets", default="chess,ataxx,go9")
    ap.add_argument("--contract", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert capi.device_count() >= 1, "needs a GPU"
    out = {"tool": "bf16_rate", "rates": [rates(k, args.regions, args.seconds) for k in args.nets.split(",") if k]}
    if args.contract:
        out["contract"] = contract()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
