#!/usr/bin/env python3
"""KZ_DTYPE_INT8 against KZ_DTYPE_F16 on the same network (bench.py measures the flagship in its own dtypes and stays as it is):
both engines of ONE calibrated model in ONE process, in interleaved timed regions (kzero_amd.benchlib.run_timed: device sync on
both sides of every region), the median of 7 regions each.  The int8 plan is a tower launch, the f16 engine's head launches and a
decode; the f16 plan of a network whose heads fit its launch is ONE launch.  So two boundaries are reported, and must not be mixed:

  decoded   the decoded host boundary — submit_packed_decoded on the four slots, the oldest waited for before its slot is used
            again: what a caller gets, launches, decode and PCIe included;
  resident  packed boards already in HBM, raw outputs left in HBM (bench.py's `--boundary resident`), two engines alternating:
            no PCIe and no decode, but still each plan's own launches;
  tower     the tower launch's own device time per batch (kz_engine_set_profiling, one engine, launches back to back).  For a
            network whose f16 plan has the heads inside, a third engine — f16 with KZ_NO_FUSED_HEADS=1: the same tower kernel,
            the heads behind it like behind the int8 tower — gives the f16 tower alone: `tower_i8_over_f16` compares like with like.

--heads adds a third engine, KZ_DTYPE_INT8_HEADS (dtype 5: the same int8 tower with the conv policy heads, the scalar head and
the decode inside its launch where it can carry them — one launch per batch like the f16 plan), to the same interleaved regions,
and the decoded and resident ratios of dtype 5 over dtype 4 and over f16: the ratio of the medians, and the smallest and largest
ratio of a region of the one to the region of the other that ran beside it (`*_regions_min_max`: the regions' spread).  Dtype 4's
kernels are untouched by dtype 5, so "5 over 4" in one process is the comparison with the library before dtype 5.  On a network
whose heads the int8 launch cannot carry (chess) dtype 5 is dtype 4's plan and the ratio is 1 within that spread.

Networks and batches: README's rows — chess 20x256 at 256, Ataxx 7x7 8x128 at 256, Go 9x9 16x128 at 2048 —, and chess128
(chess 20x128, attention head: the tower alone in either int8 dtype).  --batches 512,1024,... runs every network of --nets at
each of these batches instead of its own (the wide tiles are chosen per launch from its batch: DESIGN.md 6.2.3); every row
records the launch geometry of each engine at its batch.  The model is
calibrated on a disjoint board sample (capi.calibrate_int8, headroom 2); the rate does not depend on the calibration.

Against another build of the library (the parent commit's, built in a worktree of its own): run this tool in a second process
with KZ_LIB_PATH pointing at that build, alternating the two processes; the f16 engine's rate, whose kernels are the same in
both, is the drift check between them.

--contract adds what the int8 arithmetic costs in precision on chess 20x256 at batch 256 against the CPU oracle
(tests/oracle_lib.py), calibrated on a disjoint sample: max |delta| / scale and rms / scale per board and output tensor, and the
post-softmax max |delta p| over the whole policy, with the f16 engine's figures on the same boards beside them.  The weights are
random-init: the error of a trained network is the caller's to measure with kz_engine_set_audit.  Prints one JSON object.

    python tools/int8_rate.py [--regions 7] [--seconds 0.5] [--nets chess,ataxx,go9] [--contract] [--out profiles/int8_rate.json]
    python tools/int8_rate.py --heads     # the three engines; writes profiles/int8_heads_rate.json unless --out says otherwise
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from kzero_amd import benchlib, capi, synth  # noqa: E402
from bf16_rate import Loop  # noqa: E402  (one engine's four-slot loop of the decoded entries)

NETS = {"chess": ("chess", 20, 256, "attention", 256), "ataxx": ("ataxx-7", 8, 128, "ataxx_conv", 256),
        "go9": ("go-9", 16, 128, "conv", 2048), "chess128": ("chess", 20, 128, "attention", 256)}
OUT_HEADS = os.path.join(REPO, "profiles", "int8_heads_rate.json")
KERNEL = {"tower_resident_i8": "kz_tower_resident_i8", "tower_resident_f16": "kz_tower_resident_f16",
          "tower_resident_f16g": "kz_tower_resident_f16g"}
CALIBRATION_BOARDS, CALIBRATION_SEED, HEADROOM = 64, 7, 2.0


def calibrated(game, depth, channels, head):
    model = capi.Model(blob=synth.random_model(game, depth, channels, head, seed=3))
    bits, scalars = synth.random_boards(game, CALIBRATION_BOARDS, seed=CALIBRATION_SEED)
    return capi.calibrate_int8(model, 0, bits, scalars, headroom=HEADROOM)


def f16_heads_outside(model, batch):
    """An f16 engine whose plan keeps the heads out of the tower launch (the switch is read when the engine is made)."""
    saved = os.environ.get("KZ_NO_FUSED_HEADS")
    os.environ["KZ_NO_FUSED_HEADS"] = "1"
    try:
        return capi.Engine(model, 0, batch, capi.KZ_DTYPE_F16)
    finally:
        if saved is None:
            del os.environ["KZ_NO_FUSED_HEADS"]
        else:
            os.environ["KZ_NO_FUSED_HEADS"] = saved


class Resident:
    """Two engines alternating on device-resident inputs and outputs, as benchlib's (step, sync) pair."""

    def __init__(self, engines, bits, scalars, batch, policy_len):
        self.engines, self.batch, self.stride = engines, batch, bits.shape[1]
        self.d_bits, self.d_sin = capi.DeviceBuffer.from_host(0, bits), capi.DeviceBuffer.from_host(0, scalars)
        self.outs = [(capi.DeviceBuffer(0, batch * 5 * 4), capi.DeviceBuffer(0, batch * policy_len * 4)) for _ in engines]

    def step(self, i):
        e = i % len(self.engines)
        self.engines[e].enqueue_packed_device(self.d_bits, self.stride, self.d_sin, self.batch, *self.outs[e])

    def sync(self):
        for e in self.engines:
            e.synchronize()


def interleaved(loops, batch, regions, seconds):
    steps = {}
    for name, loop in loops.items():
        t = benchlib.run_timed(loop.step, loop.sync, 8, 8)
        steps[name] = max(16, int(seconds / (t / 8)))
    elapsed = {name: [] for name in loops}
    for _ in range(regions):  # interleaved: every engine sees the same minutes of the chip
        for name, loop in loops.items():
            elapsed[name].append(benchlib.run_timed(loop.step, loop.sync, steps[name], 4))
    out = {"_elapsed": elapsed, "_steps": steps}
    for name in loops:
        med = benchlib.median_region(elapsed[name])
        out[name] = {"steps_per_region": steps[name], "evals_per_s_median": round(steps[name] * batch / med),
                     "evals_per_s_min_max": [round(steps[name] * batch / max(elapsed[name])), round(steps[name] * batch / min(elapsed[name]))]}
    return out


def tower_time(eng, res, launches=40):
    """Microseconds per tower launch, from the engine's own event pairs."""
    eng.set_profiling(True)
    for _ in range(launches):
        eng.enqueue_packed_device(res.d_bits, res.stride, res.d_sin, res.batch, *res.outs[0])
    eng.synchronize()
    total, n = eng.kernel_time(KERNEL[eng.tower_path.replace("+heads", "")])
    eng.set_profiling(False)
    return 1e3 * total / max(n, 1), n


def ratio(result, a, b):
    """evals/s of engine a over engine b: the ratio of the medians, and the smallest and largest ratio over the regions (region i
    of a ran next to region i of b)."""
    per_region = [(result["_steps"][a] / ta) / (result["_steps"][b] / tb) for ta, tb in zip(result["_elapsed"][a], result["_elapsed"][b])]
    return round(result[a]["evals_per_s_median"] / result[b]["evals_per_s_median"], 3), [round(min(per_region), 3), round(max(per_region), 3)]


def rates(key, regions, seconds, heads=False, batch=None):
    game, depth, channels, head, own_batch = NETS[key]
    batch = batch or own_batch
    model = calibrated(game, depth, channels, head)
    rng = np.random.default_rng(1)
    bits, scalars = synth.random_boards(game, batch, seed=2)
    moves = [rng.permutation(model.info.policy_len)[:int(n)].astype(np.int32) for n in rng.integers(1, 61, size=batch)]
    out = {"network": f"{game} {depth}x{channels}", "batch": batch, "regions": regions}
    dtypes = {"int8": capi.KZ_DTYPE_INT8, "f16": capi.KZ_DTYPE_F16}
    if heads:
        dtypes["int8_heads"] = capi.KZ_DTYPE_INT8_HEADS
    engines = {name: [capi.Engine(model, 0, batch, dtype) for _ in range(2)] for name, dtype in dtypes.items()}
    out["tower_path"] = {name: e[0].tower_path for name, e in engines.items()}
    out["launches_per_batch"] = {name: model.plan(batch, dtype)[1] for name, dtype in dtypes.items()}
    out["launch_geometry"] = {name: list(e[0].launch_geometry(batch)) for name, e in engines.items()}  # [workgroups, boards per workgroup]
    decoded = {}
    for name, e in engines.items():
        offsets, idx = e[0]._csr(moves)
        decoded[name] = Loop(e[0], bits, scalars, offsets, idx)
    out["decoded"] = interleaved(decoded, batch, regions, seconds)
    resident = {name: Resident(e, bits, scalars, batch, model.info.policy_len) for name, e in engines.items()}
    out["resident"] = interleaved(resident, batch, regions, seconds)
    for boundary in ("decoded", "resident"):
        out[boundary]["int8_over_f16"] = ratio(out[boundary], "int8", "f16")[0]
        if heads:
            for a, b in (("int8_heads", "int8"), ("int8_heads", "f16")):
                out[boundary][f"{a}_over_{b}"], out[boundary][f"{a}_over_{b}_regions_min_max"] = ratio(out[boundary], a, b)
        del out[boundary]["_elapsed"], out[boundary]["_steps"]
    tower = {}
    for name, e in engines.items():
        if name == "int8_heads":  # (dtype 4's tower, bit for bit: nothing of its own to time)
            continue
        eng = e[0]
        if eng.tower_path.endswith("+heads"):
            eng = f16_heads_outside(model, batch)
        us, n = tower_time(eng, resident[name])
        tower[name] = {"tower_path": eng.tower_path, "launches": n, "us_per_launch": round(us, 2)}
    tower["tower_i8_over_f16"] = round(tower["f16"]["us_per_launch"] / tower["int8"]["us_per_launch"], 3)  # (a rate: f16 time / int8 time)
    out["tower"] = tower
    return out


def contract(batch=256):
    from tests import oracle_lib as O
    model = calibrated("chess", 20, 256, "attention")
    blob = synth.random_model("chess", 20, 256, "attention", seed=3)
    bits, scalars = synth.random_boards("chess", batch, seed=2)
    net = O.OracleNet(blob)
    s_ref, p_ref = net.forward(O.encode_input_full(bits, scalars, net.n_scalar, net.n_bool, net.h, net.w), threads=min(16, os.cpu_count() or 1))

    def softmax(x):
        e = np.exp(x - x.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)

    out = {"network": "chess 20x256 (random-init weights)", "batch": batch, "reference": "CPU oracle (f32)",
           "calibration": f"{CALIBRATION_BOARDS} other boards (seed {CALIBRATION_SEED}), headroom {HEADROOM}",
           "site_exponents": [int(e) for e in model.int8_site_exponents()],
           "scale": {"scalars": float(np.abs(s_ref).max()), "policy": float(np.abs(p_ref).max())}}
    for name, dtype in (("int8", capi.KZ_DTYPE_INT8), ("f16", capi.KZ_DTYPE_F16)):
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
    ap.add_argument("--batches", help="comma-separated batch sizes: every network at each of them instead of its own")
    ap.add_argument("--contract", action="store_true")
    ap.add_argument("--heads", action="store_true", help="a third engine, dtype 5, and its ratios over dtype 4 and f16")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert capi.device_count() >= 1, "needs a GPU"
    if args.heads and not args.out:
        args.out = OUT_HEADS
    batches = [int(b) for b in args.batches.split(",") if b] if args.batches else [None]
    out = {"tool": "int8_rate", "library": os.path.relpath(capi.LIB_PATH, REPO),
           "rates": [rates(k, args.regions, args.seconds, args.heads, b) for k in args.nets.split(",") if k for b in batches]}
    if args.contract:
        out["contract"] = contract()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
