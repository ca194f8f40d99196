#!/usr/bin/env python3
"""What the kernel that ships does to a network's stored tower tensors (include/kz_hip.h, "tower taps and error profile"): runs
kz_model_error_profile — every range site's tap of the one-launch tower against exact f32 on the same boards, reduced on the
GPU — on the positions of a position file (kzero_amd/position_file.py) or on synthetic boards, and prints per site and per dtype
max |err|, the rms error relative to the rms of the reference, and the non-finite count.

    python tools/error_profile.py --model net.kzm|net.onnx [--scalar-channels N] --positions games/file [--boards 1024]
    python tools/error_profile.py --game chess --depth 20 --channels 256 --head attention [--block-gain 64] [--boards 256]

--dtypes f16,bf16,f32split16   the arithmetics to profile (default: these three; one the model does not run is skipped with its message)
--max-batch N                  the engine size whose geometry is tapped (default: the number of boards)
--shift k1,k2,...              the same columns for kz_model_stream_shift(k) of the model, side by side: choose k by measured
                               error.  A shifted model's taps and its reference are both in shifted units, so the relative
                               columns compare across k; max |err| is multiplied back by 2^k on the sites a shift moves.
--profile-time                 the wall time of one profile call (engines created and destroyed inside), the median of 3
Prints one JSON object; --out writes it too.
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
from kzero_amd.position_file import PositionFile  # noqa: E402

DTYPES = {"f16": capi.KZ_DTYPE_F16, "f32split16": capi.KZ_DTYPE_F32_SPLIT16, "bf16": capi.KZ_DTYPE_BF16}


def rows_of(profile, k):
    """Per site: max |err| in the unshifted stream's units, rms(err) / rms(ref), the non-finite count."""
    n = len(profile)
    out = []
    for i, r in enumerate(profile):
        unit = 2.0 ** k if i < n - 1 else 1.0  # (the last site is behind the final BatchNorm: a shift does not move it)
        rel = float(np.sqrt(r["sum_sq_err"] / r["sum_sq_ref"])) if r["sum_sq_ref"] > 0 else float("nan")
        out.append({"site": str(r["site"]), "max_abs_err": float(r["max_abs_err"]) * unit, "rel_rms_err": rel,
                    "max_abs_ref": float(r["max_abs_ref"]) * unit, "count": int(r["count"]), "nonfinite": int(r["nonfinite"])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", help="a KZMODEL1 container or an ONNX file")
    ap.add_argument("--scalar-channels", type=int, help="ONNX: how many input planes are broadcast scalars")
    ap.add_argument("--positions", help="a position file (path without .json / .bin / .off)")
    ap.add_argument("--game", default="chess")
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--head", default="attention")
    ap.add_argument("--block-gain", type=float, help="synthetic model: synth.random_model's block_gain (a stream that grows)")
    ap.add_argument("--boards", type=int, default=256, help="positions to profile (the first of the file, or synthetic ones)")
    ap.add_argument("--max-batch", type=int, help="the engine size whose geometry is tapped (default: the number of boards)")
    ap.add_argument("--dtypes", default="f16,bf16,f32split16")
    ap.add_argument("--shift", default="0", help="k1,k2,...: the stream shifts to compare")
    ap.add_argument("--profile-time", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert capi.device_count() >= 1, "needs a GPU"

    if args.model:
        model = capi.Model(path=args.model, onnx_scalar_channels=args.scalar_channels)
        network = os.path.basename(args.model)
    else:
        kw = {"block_gain": args.block_gain} if args.block_gain else {}
        model = capi.Model(blob=synth.random_model(args.game, args.depth, args.channels, args.head, seed=3, **kw))
        network = f"{args.game} {args.depth}x{args.channels} (synthetic)"
    if args.positions:
        pf = PositionFile(args.positions)
        bits, scalars, _ = pf.read_boards(range(min(args.boards, len(pf))))
        source = f"{len(bits)} positions of {args.positions}"
    else:
        assert not args.model, "a model file needs --positions (synthetic boards belong to a --game)"
        bits, scalars = synth.random_boards(args.game, args.boards, seed=2)
        source = f"{args.boards} synthetic boards"
    max_batch = args.max_batch or len(bits)
    shifts = [int(k) for k in args.shift.split(",")]
    dtypes = [d.strip() for d in args.dtypes.split(",")]
    assert all(d in DTYPES for d in dtypes), f"--dtypes: any of {sorted(DTYPES)}"

    out = {"tool": "error_profile", "network": network, "boards": source, "max_batch": max_batch, "columns": []}
    for k in shifts:
        shifted = model.stream_shift(k) if k else model
        for d in dtypes:
            col = {"dtype": d, "k": k}
            try:
                col["tower_path"] = shifted.tower_taps_path(max_batch, DTYPES[d])
                col["sites"] = rows_of(shifted.error_profile(args.device, max_batch, DTYPES[d], bits, scalars), k)
                if args.profile_time:
                    times = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        shifted.error_profile(args.device, max_batch, DTYPES[d], bits, scalars)
                        times.append(time.perf_counter() - t0)
                    col["profile_call_ms"] = {"boards": len(bits), "median": round(1e3 * float(np.median(times)), 2),
                                              "min": round(1e3 * min(times), 2), "max": round(1e3 * max(times), 2)}
            except capi.KzError as e:
                col["skipped"] = str(e)
            out["columns"].append(col)

    cols = [c for c in out["columns"] if "sites" in c]
    print(f"# {network}, {source}, max_batch {max_batch}", file=sys.stderr)
    for c in out["columns"]:
        if "skipped" in c:
            print(f"# {c['dtype']} k={c['k']}: skipped: {c['skipped']}", file=sys.stderr)
    if cols:
        print(f"# {'':<14} " + " ".join(f"{c['dtype'] + ' k=' + str(c['k']):^33}" for c in cols), file=sys.stderr)
        print(f"# {'site':<14} " + " ".join(f"{'max |err|':>11} {'rms/rms':>10} {'nonfinite':>10}" for _ in cols), file=sys.stderr)
        for i in range(len(cols[0]["sites"])):
            print(f"# {cols[0]['sites'][i]['site']:<14} " +
                  " ".join(f"{c['sites'][i]['max_abs_err']:>11.4g} {c['sites'][i]['rel_rms_err']:>10.3g} {c['sites'][i]['nonfinite']:>10d}" for c in cols),
                  file=sys.stderr)
        for c in cols:
            if "profile_call_ms" in c:
                print(f"# {c['dtype']} k={c['k']}: one profile call on {len(bits)} boards: {c['profile_call_ms']['median']} ms (median of 3)", file=sys.stderr)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
