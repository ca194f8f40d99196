#!/usr/bin/env python3
"""KZ_DTYPE_INT8_ANY's per-layer plan ("board_conv_i8") against KZ_DTYPE_F16 on the same network, modelled on tools/int8_rate.py:
a dtype-8 engine and an f16 engine of ONE calibrated model in ONE process, in interleaved timed regions
(kzero_amd.benchlib.run_timed), the median of 7 regions each and the smallest and largest ratio of a region of the one to the
region of the other that ran beside it (`*_regions_min_max`: the regions' spread).  The comparison is with the f16 engine of
the same build in the same process, never with a figure from another run.  Three boundaries, not to be mixed:

  decoded   submit_packed_decoded on the four slots: what a caller gets, launches, decode and PCIe included;
  resident  packed boards already in HBM, raw outputs left in HBM, two engines alternating;
  tower     the tower layers alone, per batch, from kz_engine_kernel_time: the int8 plan's stem and 2 x depth block launches
            against the f16 plan's tower launches (its per-layer launches, or its one-launch tower with the heads kept outside).

Networks: Go 19x19 40x256 at batch 512 (BASELINE configs[4]) and Go 9x9 16x256 at 2048.  The model is calibrated on a disjoint
board sample (capi.calibrate_int8, 64 boards, headroom 2); the rate does not depend on the calibration.

--contract adds the error of both engines against the exact-f32 engine on Go 19x19 40x256, 64 evaluated boards, calibrated on
64 other boards with headroom 2 (random-init weights: the error of a trained network is the caller's to measure with
kz_engine_set_audit).  Writes profiles/int8_board_rate.json unless --out says otherwise.

    python tools/int8_board_rate.py [--regions 7] [--seconds 0.5] [--nets go19,go9] [--contract] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from kzero_amd import capi, synth  # noqa: E402
from bf16_rate import Loop  # noqa: E402
from int8_rate import CALIBRATION_BOARDS, CALIBRATION_SEED, HEADROOM, Resident, calibrated, f16_heads_outside, interleaved, ratio  # noqa: E402

NETS = {"go19": ("go-19", 40, 256, "conv", 512), "go9": ("go-9", 16, 256, "conv", 2048)}
OUT = os.path.join(REPO, "profiles", "int8_board_rate.json")
TOWER_KERNELS = {"board_conv_i8": ("kz_board_conv_i8_stem", "kz_board_conv_i8"), "board_conv_f16": ("kz_board_conv_f16",),
                 "tower_resident_f16g": ("kz_tower_resident_f16g",), "tower_resident_f16": ("kz_tower_resident_f16",),
                 "conv_igemm_f16": ("kz_conv_igemm_f16",)}


def tower_time(eng, res, batches=20):
    """Microseconds of the tower's launches per batch, from the engine's own event pairs."""
    eng.set_profiling(True)
    for _ in range(batches):
        eng.enqueue_packed_device(res.d_bits, res.stride, res.d_sin, res.batch, *res.outs[0])
    eng.synchronize()
    total, launches = 0.0, 0
    for kernel in TOWER_KERNELS[eng.tower_path]:
        t, n = eng.kernel_time(kernel)
        total, launches = total + t, launches + n
    eng.set_profiling(False)
    return 1e3 * total / batches, launches // batches


def rates(key, regions, seconds):
    game, depth, channels, head, batch = NETS[key]
    model = calibrated(game, depth, channels, head)
    rng = np.random.default_rng(1)
    bits, scalars = synth.random_boards(game, batch, seed=2)
    moves = [rng.permutation(model.info.policy_len)[:int(n)].astype(np.int32) for n in rng.integers(1, 61, size=batch)]
    out = {"network": f"{game} {depth}x{channels}", "batch": batch, "regions": regions}
    dtypes = {"int8": capi.KZ_DTYPE_INT8_ANY, "f16": capi.KZ_DTYPE_F16}
    engines = {name: [capi.Engine(model, 0, batch, dtype) for _ in range(2)] for name, dtype in dtypes.items()}
    out["tower_path"] = {name: e[0].tower_path for name, e in engines.items()}
    out["launches_per_batch"] = {name: model.plan(batch, dtype)[1] for name, dtype in dtypes.items()}
    out["launch_geometry"] = {name: list(e[0].launch_geometry(batch)) for name, e in engines.items()}
    decoded = {}
    for name, e in engines.items():
        offsets, idx = e[0]._csr(moves)
        decoded[name] = Loop(e[0], bits, scalars, offsets, idx)
    out["decoded"] = interleaved(decoded, batch, regions, seconds)
    resident = {name: Resident(e, bits, scalars, batch, model.info.policy_len) for name, e in engines.items()}
    out["resident"] = interleaved(resident, batch, regions, seconds)
    for boundary in ("decoded", "resident"):
        r, spread = ratio(out[boundary], "int8", "f16")
        out[boundary]["int8_over_f16"], out[boundary]["int8_over_f16_regions_min_max"] = r, spread
        # above 1 by more than the regions' spread, or not: said next to the number
        out[boundary]["int8_faster_beyond_the_spread"] = bool(spread[0] > 1.0)
        del out[boundary]["_elapsed"], out[boundary]["_steps"]
    tower = {}
    for name, e in engines.items():
        eng = e[0]
        if eng.tower_path.endswith("+heads"):
            eng = f16_heads_outside(model, batch)
        us, n = tower_time(eng, resident[name])
        tower[name] = {"tower_path": eng.tower_path, "launches_per_batch": n, "us_per_batch": round(us, 2)}
    tower["tower_i8_over_f16"] = round(tower["f16"]["us_per_batch"] / tower["int8"]["us_per_batch"], 3)  # (a rate: f16 time / int8 time)
    out["tower"] = tower
    return out


def contract(boards=64):
    game, depth, channels, head, _ = NETS["go19"]
    model = calibrated(game, depth, channels, head)
    bits, scalars = synth.random_boards(game, boards, seed=2)
    s_ref, p_ref = capi.Engine(model, 0, boards, capi.KZ_DTYPE_F32).eval_packed(bits, scalars)
    out = {"network": f"{game} {depth}x{channels} (random-init weights)", "boards": boards, "reference": "the exact-f32 engine of the same model",
           "calibration": f"{CALIBRATION_BOARDS} other boards (seed {CALIBRATION_SEED}), headroom {HEADROOM}",
           "site_exponents_min_max": [int(min(model.int8_site_exponents())), int(max(model.int8_site_exponents()))],
           "scale": {"scalars": float(np.abs(s_ref).max()), "policy": float(np.abs(p_ref).max())}}

    def softmax(x):
        e = np.exp(x - x.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)

    for name, dtype in (("int8", capi.KZ_DTYPE_INT8_ANY), ("f16", capi.KZ_DTYPE_F16)):
        s, p = capi.Engine(model, 0, boards, dtype).eval_packed(bits, scalars)
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
    ap.add_argument("--nets", default="go19,go9")
    ap.add_argument("--contract", action="store_true")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    assert capi.device_count() >= 1, "needs a GPU"
    out = {"tool": "int8_board_rate", "library": os.path.relpath(capi.LIB_PATH, REPO),
           "rates": [rates(k, args.regions, args.seconds) for k in args.nets.split(",") if k]}
    if args.contract:
        out["contract"] = contract()
    text = json.dumps(out, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
