#!/usr/bin/env python3
"""How much f16 headroom a network has, and the stream shift that gives it some (include/kz_hip.h, "stream shift and range
profile"): runs kz_model_range_profile — max |x| of every tensor an f16 / split16 tower kernel stores, exact f32 on the GPU — on
the positions of a position file (kzero_amd/position_file.py) or on synthetic boards, prints the per-site table (max, fraction of
65504) and the suggested k = max(0, ceil(log2(m / 65504)) + headroom_bits), m the maximum over the sites a shift moves.

    python tools/range_profile.py --model net.kzm|net.onnx [--scalar-channels N] --positions games/file [--boards 1024]
    python tools/range_profile.py --game chess --depth 20 --channels 256 --head attention [--block-gain 64] [--boards 256]

--check  evaluates the boards with the f16 engine of the SHIFTED model (the suggested k, or --k) through the decoded status entry,
         with the shadow audit against exact f32 on every batch: the status words per kind and the audit's statistics.
--rate   shifted against unshifted evals/s of the f16 engine (--dtype: another arithmetic) at --batch: the decoded host-boundary
         rate on the four slots, both models in ONE process, interleaved timed regions, the median of --regions each — and the
         unshifted model's own max - min spread over its regions, the bar the difference has to clear.
--profile-time  the wall time of the profile call itself (engine creation included), the median of 5 calls.
--fast   the table from kz_model_range_profile_fast: the same profile inside the one-launch exact-f32 tower where that kernel
         takes the network (the JSON names the path).  With --rate it is the PROFILE's rate that is measured instead of an
         engine's: the fast entry against the per-layer entry on the same boards in one process, interleaved calls (engine
         creation included), the median of 5 each, boards per second, and whether the fast call's median is below the other's.
         --hold-f32 keeps an ordinary exact-f32 engine of the model alive meanwhile (what KZ_HIP_RANGE_FALLBACK=1 does in a
         self-play run): the fast entry's internal engine then finds its weight stream in the cache instead of packing it.
--hist   the range histogram (kz_model_range_histogram; with --fast kz_model_range_histogram_fast): per site, what
         capi.shift_report says of the rule's k and of k - 2 and k + 2 — the shares of the stored values that are zero, beyond
         f16, in f16's top binade, f16 subnormals, flushed, and without a split16 lo half.  With --rate the four entries are
         timed instead of an engine: both histogram entries next to both max entries on the same boards in one process,
         interleaved calls, the median of 5 each, with an exact-f32 engine of the model alive (the weights are cached).
         --max-lib takes the two max entries from ANOTHER build of the library (tools/build_rev_lib.sh: the parent commit's),
         loaded beside this one with a model and a held engine of its own.
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

from kzero_amd import benchlib, capi, synth  # noqa: E402
from kzero_amd.position_file import PositionFile  # noqa: E402

DTYPES = {"f16": capi.KZ_DTYPE_F16, "f32split16": capi.KZ_DTYPE_F32_SPLIT16, "f32": capi.KZ_DTYPE_F32, "bf16": capi.KZ_DTYPE_BF16}


class Loop:
    """One engine's four-slot loop as benchlib's (step, sync) pair (tools/bf16_rate.py)."""

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


def random_moves(policy_len, n, seed=1):
    rng = np.random.default_rng(seed)
    return [rng.permutation(policy_len)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=n)]


def check(model, k, bits, scalars, moves, device):
    """The f16 engine of the shifted model on the profiled boards: status words and the audit against exact f32."""
    eng = capi.Engine(model.stream_shift(k), device, min(len(bits), 256), capi.KZ_DTYPE_F16)
    audit_boards = min(eng.max_batch, 64)
    eng.set_audit(capi.KZ_DTYPE_F32, 1, audit_boards)
    counts = {"ok": 0, "bad_decode": 0, "nonfinite": 0}
    for lo in range(0, len(bits), eng.max_batch):
        hi = min(lo + eng.max_batch, len(bits))
        _, _, status = eng.eval_packed_decoded_status(bits[lo:hi], scalars[lo:hi], moves[lo:hi])
        counts["ok"] += int((status == 0).sum())
        counts["bad_decode"] += int(((status & capi.KZ_BOARD_BAD_DECODE) != 0).sum())
        counts["nonfinite"] += int(((status & capi.KZ_BOARD_NONFINITE) != 0).sum())
    a = eng.audit_stats()
    return {"k": k, "tower_path": eng.tower_path, "boards": len(bits), "status": counts,
            "audit_vs_f32": {"boards": a.boards, "moves": a.moves, "skipped": a.skipped, "max_abs_value": a.max_abs_value.tolist(),
                             "max_abs_prob": float(a.max_abs_prob), "rms_value": a.rms_value.tolist(), "rms_prob": a.rms_prob}}


def rate(model, k, bits, scalars, moves, device, dtype, batch, regions, seconds):
    pick = np.arange(batch) % len(bits)
    bits, scalars, moves = np.ascontiguousarray(bits[pick]), np.ascontiguousarray(scalars[pick]), [moves[i] for i in pick]
    loops, paths = {}, {}
    for name, m in (("unshifted", model), ("shifted", model.stream_shift(k))):
        eng = capi.Engine(m, device, batch, DTYPES[dtype])
        offsets, idx = eng._csr(moves)
        loops[name], paths[name] = Loop(eng, bits, scalars, offsets, idx), eng.tower_path
    steps = {}
    for name, loop in loops.items():
        t = benchlib.run_timed(loop.step, loop.sync, 8, 8)
        steps[name] = max(16, int(seconds / (t / 8)))
    elapsed = {name: [] for name in loops}
    for _ in range(regions):  # interleaved: both models see the same minutes of the chip
        for name, loop in loops.items():
            elapsed[name].append(benchlib.run_timed(loop.step, loop.sync, steps[name], 4))
    out = {"k": k, "dtype": dtype, "batch": batch, "regions": regions}
    for name in loops:
        per_region = [steps[name] * batch / t for t in elapsed[name]]
        out[name] = {"tower_path": paths[name], "steps_per_region": steps[name],
                     "evals_per_s_median": round(steps[name] * batch / benchlib.median_region(elapsed[name])),
                     "evals_per_s_min_max": [round(min(per_region)), round(max(per_region))]}
    lo, hi = out["unshifted"]["evals_per_s_min_max"]
    out["unshifted_spread"] = hi - lo
    out["shifted_minus_unshifted"] = out["shifted"]["evals_per_s_median"] - out["unshifted"]["evals_per_s_median"]
    out["inside_the_spread"] = abs(out["shifted_minus_unshifted"]) <= out["unshifted_spread"]
    return out


def profile_rate(model, bits, scalars, device, calls=5, hold_f32=False):
    """Both profile entries on the same boards, interleaved: wall time per call (engine creation included) and boards/s."""
    held = capi.Engine(model, device, 64, capi.KZ_DTYPE_F32) if hold_f32 else None
    entries = {"fast": model.range_profile_fast, "per_layer": model.range_profile}
    for fn in entries.values():  # (code objects loaded, weights packed once: what a second network of a run pays)
        fn(device, bits, scalars)
    times = {name: [] for name in entries}
    for _ in range(calls):
        for name, fn in entries.items():
            t0 = time.perf_counter()
            fn(device, bits, scalars)
            times[name].append(time.perf_counter() - t0)
    out = {"boards": len(bits), "calls": calls, "fast_path": model.range_profile_fast_path(),
           "f32_engine_held": held.tower_path if held else None}
    for name, t in times.items():
        med = float(np.median(t))
        out[name] = {"ms_median": round(1e3 * med, 3), "ms_min": round(1e3 * min(t), 3), "ms_max": round(1e3 * max(t), 3),
                     "boards_per_s_median": round(len(bits) / med)}
    out["fast_below_per_layer"] = out["fast"]["ms_median"] < out["per_layer"]["ms_median"]
    return out


SHARES = ("zero", "nonfinite", "f16_over", "f16_top", "f16_subnormal", "f16_flushed", "split_lo_subnormal", "clamped_low",
          "clamped_high")


def hist_report(hist, sites, k):
    """shift_report for k - 2, k, k + 2 (inside [-24, 24]) as shares of each site's elements."""
    out = []
    for kk in sorted({max(-24, min(24, k + d)) for d in (-2, 0, 2)}):
        r = capi.shift_report(hist, kk)
        out.append({"k": kk, "sites": [{"site": s, "elements": int(r["total"][i]),
                                        **{f: float(r[f][i]) / max(int(r["total"][i]), 1) for f in SHARES}}
                                       for i, s in enumerate(sites)]})
    return out


class OtherLib:
    """The two max entries of another build of the library: its own model of the same blob and its own held exact-f32 engine."""

    def __init__(self, path, blob, device):
        C = capi.C
        self.lib, self.device = C.CDLL(path), device
        for name in ("kz_model_load_memory", "kz_model_range_sites", "kz_model_range_profile", "kz_model_range_profile_fast",
                     "kz_engine_create"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = capi.SIGNATURES[name]
        self.lib.kz_last_error.restype = C.c_char_p
        self.model, self.engine = C.c_void_p(), C.c_void_p()
        self.check(self.lib.kz_model_load_memory(blob, len(blob), C.byref(self.model)))
        self.check(self.lib.kz_engine_create(self.model, device, 64, capi.KZ_DTYPE_F32, C.byref(self.engine)))
        n = C.c_int()
        self.check(self.lib.kz_model_range_sites(self.model, C.byref(n)))
        self.site_max = np.zeros(n.value, np.float32)

    def check(self, rc):
        assert rc == 0, self.lib.kz_last_error().decode()

    def entry(self, name):
        fn = getattr(self.lib, name)

        def call(device, bits, scalars):
            self.check(fn(self.model, device, bits.ctypes.data, bits.shape[1], scalars.ctypes.data, bits.shape[0],
                          self.site_max.ctypes.data, None))
        return call


def hist_rate(model, blob, bits, scalars, device, max_lib=None, calls=5):
    """The two histogram entries and the two max entries on the same boards, interleaved, an exact-f32 engine held: wall time
    per call (engine creation included) and boards/s."""
    held = capi.Engine(model, device, 64, capi.KZ_DTYPE_F32)
    bits, scalars = np.ascontiguousarray(bits, np.uint8), np.ascontiguousarray(scalars, np.float32)
    other = OtherLib(max_lib, blob, device) if max_lib else None
    entries = {"hist_fast": lambda d, b, s: model.range_histogram(d, b, s, fast=True),
               "hist_per_layer": lambda d, b, s: model.range_histogram(d, b, s, fast=False),
               "max_fast": other.entry("kz_model_range_profile_fast") if other else model.range_profile_fast,
               "max_per_layer": other.entry("kz_model_range_profile") if other else model.range_profile}
    for fn in entries.values():
        fn(device, bits, scalars)
    times = {name: [] for name in entries}
    for _ in range(calls):
        for name, fn in entries.items():
            t0 = time.perf_counter()
            fn(device, bits, scalars)
            times[name].append(time.perf_counter() - t0)
    out = {"boards": len(bits), "calls": calls, "fast_path": model.range_profile_fast_path(), "f32_engine_held": held.tower_path,
           "max_entries_from": max_lib or "this library"}
    for name, t in times.items():
        med = float(np.median(t))
        out[name] = {"ms_median": round(1e3 * med, 3), "ms_min": round(1e3 * min(t), 3), "ms_max": round(1e3 * max(t), 3),
                     "boards_per_s_median": round(len(bits) / med)}
    out["hist_fast_below_max_per_layer"] = out["hist_fast"]["ms_median"] < out["max_per_layer"]["ms_median"]
    out["hist_fast_over_max_fast"] = round(out["hist_fast"]["ms_median"] / out["max_fast"]["ms_median"], 3)
    out["hist_per_layer_over_max_per_layer"] = round(out["hist_per_layer"]["ms_median"] / out["max_per_layer"]["ms_median"], 3)
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
    ap.add_argument("--headroom", type=int, default=2, help="bits of headroom: unseen positions can be larger than these")
    ap.add_argument("--k", type=int, help="shift for --check / --rate instead of the suggested one")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--rate", action="store_true")
    ap.add_argument("--profile-time", action="store_true")
    ap.add_argument("--fast", action="store_true", help="profile through kz_model_range_profile_fast; with --rate: the profile's own rate")
    ap.add_argument("--hold-f32", action="store_true", help="--rate --fast: an exact-f32 engine of the model stays alive (shared weight stream)")
    ap.add_argument("--hist", action="store_true", help="the range histogram and what shift_report says of k - 2, k, k + 2; with --rate: the entries' rates")
    ap.add_argument("--max-lib", help="--hist --rate: another build of the library for the two max entries (the parent commit's)")
    ap.add_argument("--dtype", default="f16", choices=sorted(DTYPES))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.5, help="length of a timed region")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert capi.device_count() >= 1, "needs a GPU"

    if args.model:
        model = capi.Model(path=args.model, onnx_scalar_channels=args.scalar_channels)
        network, blob = os.path.basename(args.model), None
    else:
        kw = {"block_gain": args.block_gain} if args.block_gain else {}
        blob = synth.random_model(args.game, args.depth, args.channels, args.head, seed=3, **kw)
        model = capi.Model(blob=blob)
        network = f"{args.game} {args.depth}x{args.channels} (synthetic)"
    if args.positions:
        pf = PositionFile(args.positions)
        bits, scalars, moves = pf.read_boards(range(min(args.boards, len(pf))))
        source = f"{len(bits)} positions of {args.positions}"
    else:
        assert not args.model, "a model file needs --positions (synthetic boards belong to a --game)"
        bits, scalars = synth.random_boards(args.game, args.boards, seed=2)
        moves = random_moves(model.info.policy_len, args.boards)
        source = f"{args.boards} synthetic boards"

    sites = model.range_sites()
    profile = model.range_profile_fast if args.fast else model.range_profile
    site_max, board_max = profile(args.device, bits, scalars)
    m = float(site_max[:-1].max())
    suggested = capi.shift_for(m, args.headroom) if np.isfinite(m) else None
    out = {"tool": "range_profile", "network": network, "boards": source,
           "sites": [{"site": s, "max_abs": float(v), "of_65504": float(v) / capi.F16_MAX, "shift_moves_it": i < len(sites) - 1}
                     for i, (s, v) in enumerate(zip(sites, site_max))],
           "stream_max": m, "boards_beyond_65504": int((board_max > capi.F16_MAX).sum()), "headroom_bits": args.headroom,
           "suggested_k": suggested}
    if args.fast:
        out["profile_path"] = model.range_profile_fast_path()
    print(f"# {network}, {source}", file=sys.stderr)
    print(f"# {'site':<14} {'max |x|':>14} {'of 65504':>10}", file=sys.stderr)
    for row in out["sites"]:
        print(f"# {row['site']:<14} {row['max_abs']:>14.6g} {row['of_65504']:>10.3g}" + ("" if row["shift_moves_it"] else "   (a shift does not move it)"),
              file=sys.stderr)
    print(f"# stream max {m:.6g}, {out['boards_beyond_65504']} of {len(bits)} boards beyond 65504: suggested k = {suggested} "
          f"({args.headroom} bits of headroom)", file=sys.stderr)
    if args.hist:
        k_for = args.k if args.k is not None else suggested if suggested is not None else 0
        hist = model.range_histogram(args.device, bits, scalars, fast=args.fast)
        out["histogram"] = {"entry": "kz_model_range_histogram_fast" if args.fast else "kz_model_range_histogram", "k": k_for,
                            "reports": hist_report(hist, sites, k_for)}
        for rep in out["histogram"]["reports"]:
            print(f"# k = {rep['k']}: share of each site's stored values", file=sys.stderr)
            print(f"# {'site':<14} " + " ".join(f"{f[:13]:>13}" for f in SHARES), file=sys.stderr)
            for row in rep["sites"]:
                print(f"# {row['site']:<14} " + " ".join(f"{row[f]:>13.3g}" for f in SHARES), file=sys.stderr)
        if args.rate:
            if args.max_lib and blob is None:
                blob = open(args.model, "rb").read()
            out["histogram_rate"] = hist_rate(model, blob, bits, scalars, args.device, args.max_lib)
            args.rate = False
    if args.profile_time:
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            profile(args.device, bits, scalars)
            times.append(time.perf_counter() - t0)
        out["profile_call_ms"] = {"boards": len(bits), "median": round(1e3 * float(np.median(times)), 2), "min": round(1e3 * min(times), 2),
                                  "max": round(1e3 * max(times), 2)}
    if args.rate and args.fast:
        out["profile_rate"] = profile_rate(model, bits, scalars, args.device, hold_f32=args.hold_f32)
        args.rate = False
    k = args.k if args.k is not None else suggested
    if args.check or args.rate:
        assert k is not None, "the stream is not finite on these boards: no shift repairs that"
    if args.check:
        out["check"] = check(model, k, bits, scalars, moves, args.device)
    if args.rate:
        out["rate"] = rate(model, k, bits, scalars, moves, args.device, args.dtype, args.batch, args.regions, args.seconds)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
