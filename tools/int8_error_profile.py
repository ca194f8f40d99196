#!/usr/bin/env python3
"""What a headroom costs an int8 network, per site (include/kz_hip.h, "int8 taps and error profile"): per headroom the model is
calibrated with capi.calibrate_int8 on one set of positions and kz_model_int8_error_profile runs on ANOTHER — every stored int8
image (q * 2^e_s) and the f16 stream value beside it against exact f32 on the same boards, reduced on the GPU, with the count of
image elements at the clamp and of reference values an ideal int8 image would clamp.  Prints the headrooms side by side.

    python tools/int8_error_profile.py --model net.kzm|net.onnx [--scalar-channels N] --positions games/file [--boards 1024]
    python tools/int8_error_profile.py --synthetic chess 20 256 attention [--boards 256]

--dtype 4|5|8            the int8 dtype whose tap engine runs (default 4; 5 taps what 4 taps; 8 the per-layer kernel where 5 has no plan)
--headroom h1,h2,...     the headrooms over the calibration boards' site maxima, one column each (default 1,2,4)
--calibrate-on N         boards to calibrate on: the N positions BEHIND the evaluated ones of the file, or N other synthetic boards
--max-batch N            the engine size whose geometry is tapped (default: the number of boards)
--profile-time           the wall time of one profile call (engines created and destroyed inside), the median of 3
--json FILE              writes the records too
--fake                   no GPU: made-up records through the same parsing and printing (tests/test_int8_taps_abi.py)
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

FIELDS = ("max_abs_err", "sum_sq_err", "sum_sq_ref", "max_abs_ref", "count", "nonfinite")


def rel(part):
    """rms(err) / rms(ref) of one kz_site_error; None where nothing was compared."""
    return float(np.sqrt(part["sum_sq_err"] / part["sum_sq_ref"])) if part["count"] and part["sum_sq_ref"] > 0 else None


def rows_of(profile):
    """Per site: the exponent, both records with their rms ratio, and the two clamp shares of the image's elements."""
    out = []
    for r in profile:
        image = {f: (int(r["image"][f]) if f in ("count", "nonfinite") else float(r["image"][f])) for f in FIELDS}
        stream = {f: (int(r["stream"][f]) if f in ("count", "nonfinite") else float(r["stream"][f])) for f in FIELDS}
        n = image["count"] + image["nonfinite"]
        out.append({"site": str(r["site"]), "exponent": int(r["exponent"]), "image": image, "stream": stream,
                    "image_rel_rms_err": rel(image), "stream_rel_rms_err": rel(stream),
                    "at_clamp": int(r["at_clamp"]), "ref_beyond": int(r["ref_beyond"]),
                    "at_clamp_share": int(r["at_clamp"]) / n if n else None, "ref_beyond_share": int(r["ref_beyond"]) / n if n else None})
    return out


def fake_profile(headroom, depth=2, elements=4096):
    """Records of the library's shape without a GPU: mid sites have no stream, the last site no image."""
    n = 2 * depth + 1
    names = ["tower.0"] + [s for i in range(1, depth + 1) for s in (f"tower.{i}.mid", f"tower.{i}")]
    names[-1] = f"tower.{depth + 1}"
    prof = np.zeros(n, np.dtype([("site", "U24")] + capi.INT8_SITE_ERROR_DTYPE.descr))
    prof["site"] = names
    for i in range(n):
        e = int(np.ceil(np.log2(headroom))) - 3
        if i < n - 1:
            prof[i]["image"] = (2.0 ** (e - 1), elements * 4.0 ** e / 12, elements * 1.0, 127 * 2.0 ** e / headroom, elements, 0)
            prof[i]["at_clamp"] = int(elements / 64 / headroom)
            prof[i]["ref_beyond"] = int(elements / 128 / headroom) if headroom < 2 else 0
            prof[i]["exponent"] = e
        if i % 2 == 0:
            prof[i]["stream"] = (2.0 ** -8, elements * 4.0 ** -9, elements * 1.0, 16.0, elements, 0)
    return prof


def fmt(v, width, spec):
    """A right-aligned cell; "-" where the site has no such tensor."""
    return (format(v, spec) if v is not None else "-").rjust(width)


def print_table(out, file=None):
    file = file or sys.stderr
    cols = [c for c in out["columns"] if "sites" in c]
    print(f"# {out['network']}, {out['boards']}, calibrated on {out['calibrated_on']}, dtype {out['dtype']}, max_batch {out['max_batch']}", file=file)
    for c in out["columns"]:
        if "skipped" in c:
            print(f"# headroom {c['headroom']:g}: skipped: {c['skipped']}", file=file)
    if not cols:
        return
    width = 60
    print(f"# {'':<14} " + " ".join(f"{'headroom ' + format(c['headroom'], 'g') + ' (' + c.get('tower_path', '') + ')':^{width}}" for c in cols), file=file)
    head = f"{'e':>4} {'img rms/rms':>11} {'x rms/rms':>10} {'max |err|':>10} {'at clamp':>9} {'ref beyond':>10}"
    print(f"# {'site':<14} " + " ".join(f"{head:<{width}}" for _ in cols), file=file)
    for i in range(len(cols[0]["sites"])):
        cells = []
        for c in cols:
            s = c["sites"][i]
            has_image = s["image"]["count"] + s["image"]["nonfinite"] > 0
            cell = (f"{fmt(s['exponent'] if has_image else None, 4, 'd')} {fmt(s['image_rel_rms_err'], 11, '.3g')} {fmt(s['stream_rel_rms_err'], 10, '.3g')} "
                    f"{fmt((s['image'] if has_image else s['stream'])['max_abs_err'], 10, '.4g')} {fmt(s['at_clamp_share'], 9, '.2%')} {fmt(s['ref_beyond_share'], 10, '.2%')}")
            cells.append(f"{cell:<{width}}")
        print(f"# {cols[0]['sites'][i]['site']:<14} " + " ".join(cells), file=file)
    for c in cols:
        if "profile_call_ms" in c:
            print(f"# headroom {c['headroom']:g}: one profile call on {c['profile_call_ms']['boards']} boards: {c['profile_call_ms']['median']} ms (median of 3)", file=file)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", help="a KZMODEL1 container or an ONNX file")
    ap.add_argument("--scalar-channels", type=int, help="ONNX: how many input planes are broadcast scalars")
    ap.add_argument("--positions", help="a position file (path without .json / .bin / .off)")
    ap.add_argument("--synthetic", nargs=4, metavar=("GAME", "DEPTH", "CHANNELS", "HEAD"), help="a random-init network and synthetic boards")
    ap.add_argument("--boards", type=int, default=256, help="positions to profile (the first of the file, or synthetic ones)")
    ap.add_argument("--calibrate-on", type=int, default=64, help="other boards than the evaluated ones, to calibrate on")
    ap.add_argument("--dtype", type=int, default=4, choices=(4, 5, 8))
    ap.add_argument("--headroom", default="1,2,4", help="h1,h2,...: the headrooms to compare")
    ap.add_argument("--max-batch", type=int, help="the engine size whose geometry is tapped (default: the number of boards)")
    ap.add_argument("--profile-time", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", help="write the records to this file")
    ap.add_argument("--fake", action="store_true", help="no GPU: made-up records through the same printing")
    args = ap.parse_args(argv)
    headrooms = [float(h) for h in args.headroom.split(",")]
    assert headrooms and all(h > 0 for h in headrooms), "--headroom: positive numbers"
    assert args.boards >= 1 and args.calibrate_on >= 1
    assert bool(args.model) != bool(args.synthetic), "one of --model (with --positions) and --synthetic"

    if args.synthetic:
        game, depth, channels, head = args.synthetic[0], int(args.synthetic[1]), int(args.synthetic[2]), args.synthetic[3]
        network = f"{game} {depth}x{channels} (synthetic)"
        source, calibrated_on = f"{args.boards} synthetic boards", f"{args.calibrate_on} other synthetic boards"
    else:
        assert args.positions, "a model file needs --positions (synthetic boards belong to --synthetic)"
        network = os.path.basename(args.model)
    if not args.fake:
        assert capi.device_count() >= 1, "needs a GPU"
        if args.synthetic:
            model = capi.Model(blob=synth.random_model(game, depth, channels, head, seed=3))
            bits, scalars = synth.random_boards(game, args.boards, seed=2)
            cal_bits, cal_scalars = synth.random_boards(game, args.calibrate_on, seed=7)
        else:
            from kzero_amd.position_file import PositionFile
            model = capi.Model(path=args.model, onnx_scalar_channels=args.scalar_channels)
            pf = PositionFile(args.positions)
            n = min(args.boards, len(pf))
            assert len(pf) > n, "the file has no positions behind the evaluated ones to calibrate on"
            bits, scalars, _ = pf.read_boards(range(n))
            cal = range(n, min(n + args.calibrate_on, len(pf)))
            cal_bits, cal_scalars, _ = pf.read_boards(cal)
            source, calibrated_on = f"{len(bits)} positions of {args.positions}", f"the {len(cal)} positions behind them"
        n_boards = len(bits)
    else:
        if not args.synthetic:
            source, calibrated_on = f"{args.boards} positions of {args.positions}", f"the {args.calibrate_on} positions behind them"
        n_boards = args.boards
    max_batch = args.max_batch or n_boards

    out = {"tool": "int8_error_profile", "network": network, "boards": source, "calibrated_on": calibrated_on, "dtype": args.dtype,
           "max_batch": max_batch, "columns": []}
    for h in headrooms:
        col = {"headroom": h}
        try:
            if args.fake:
                col["tower_path"] = "tower_resident_i8"
                col["sites"] = rows_of(fake_profile(h))
            else:
                quant = capi.calibrate_int8(model, args.device, cal_bits, cal_scalars, headroom=h)
                col["tower_path"] = quant.int8_taps_path(max_batch, args.dtype)
                col["sites"] = rows_of(quant.int8_error_profile(args.device, max_batch, args.dtype, bits, scalars))
                if args.profile_time:
                    times = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        quant.int8_error_profile(args.device, max_batch, args.dtype, bits, scalars)
                        times.append(time.perf_counter() - t0)
                    col["profile_call_ms"] = {"boards": n_boards, "median": round(1e3 * float(np.median(times)), 2),
                                              "min": round(1e3 * min(times), 2), "max": round(1e3 * max(times), 2)}
        except capi.KzError as e:
            col["skipped"] = str(e)
        out["columns"].append(col)

    print_table(out)
    text = json.dumps(out, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")
    return out


if __name__ == "__main__":
    main()
