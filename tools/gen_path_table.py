#!/usr/bin/env python3
"""Which path a network takes: the table of DESIGN.md §5.0, generated from the library's own selector.

`kz_model_plan` (include/kz_hip.h) is the host logic `kz_engine_create` runs — no GPU needed — so this script runs in the
build container.  It writes tests/golden/path_table.json:

  "paths":   {sweep case id: {"f32" | "f16" | "parity": tower path}}   for tests/test_shape_sweep.py (-m gpu)
  "lattice": rows (game, squares, c_in, channels, head) x (f32, f16, parity) -> tower path, launches per batch
             at max_batch 256, for the DESIGN table
  "switches": every sweep case x (f32, f16, f32split16) x max_batch (1, 8, 256, 2048) x the environment switches that
             steer the selector (none, or one of SWITCH_SETS) -> "path launches", or "refused".  Compact: the distinct
             entries once ("values"), and per case one character per entry, an index into them, in the order
             dtype, max_batch, switch set (the innermost)

tests/golden/path_table_bf16.json (--bf16) is the same column for the bf16 arithmetic (KZ_DTYPE_BF16), in a file of its own so
that the table above keeps its shape: {"max_batch": [...], "cases": {sweep case id: ["path launches" | "refused", ...]}},
no switch sets (KZ_NO_FUSED_HEADS is the only switch that arithmetic reads); tests/test_bf16_plan.py recomputes it.

tests/golden/path_table_int8.json (--int8) is that column for the int8 arithmetic (KZ_DTYPE_INT8) on the calibrated model
(every site maximum 1: the plan does not depend on the values): the same shape, with "uncalibrated" beside it — what the model
as loaded is told, always "refused" — and "no calibration" where kz_model_quantize_int8 itself refuses the network;
tests/test_int8_api.py recomputes it.

tests/golden/path_table_int8_heads.json (--int8-heads) is the same table, cases and batches for KZ_DTYPE_INT8_HEADS (dtype 5):
"tower_resident_i8+heads 1" where the int8 launch carries the conv heads, dtype 4's entry everywhere else;
tests/test_int8_heads_api.py recomputes both.

tests/golden/path_table_int8_any.json (--int8-any) is the same table for KZ_DTYPE_INT8_ANY (dtype 8): dtype 5's entry wherever it
has one, "board_conv_i8 launches" where the per-layer int8 kernel takes over; tests/test_int8_any_api.py recomputes it.

tests/test_path_table.py recomputes both from the built library and fails on any difference: a change of a support
predicate has to come with a regenerated table (python tools/gen_path_table.py) and shows up in the diff.

    python tools/gen_path_table.py            # rewrite the JSON
    python tools/gen_path_table.py --bf16     # rewrite tests/golden/path_table_bf16.json
    python tools/gen_path_table.py --int8     # rewrite tests/golden/path_table_int8.json
    python tools/gen_path_table.py --int8-heads  # rewrite tests/golden/path_table_int8_heads.json
    python tools/gen_path_table.py --int8-any    # rewrite tests/golden/path_table_int8_any.json
    python tools/gen_path_table.py --md       # print the DESIGN table (with measured rates from a sweep record, if given:
                                              #   --rates profiles/r4/shape_sweep.json)
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from kzero_amd import capi, synth  # noqa: E402
from tests import sweep_cases  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "path_table.json")
OUT_BF16 = os.path.join(REPO, "tests", "golden", "path_table_bf16.json")
OUT_INT8 = os.path.join(REPO, "tests", "golden", "path_table_int8.json")
OUT_INT8_HEADS = os.path.join(REPO, "tests", "golden", "path_table_int8_heads.json")
OUT_INT8_ANY = os.path.join(REPO, "tests", "golden", "path_table_int8_any.json")
MAX_BATCH = 256
DTYPES = {"f32": capi.KZ_DTYPE_F32, "f16": capi.KZ_DTYPE_F16, "f32split16": capi.KZ_DTYPE_F32_SPLIT16}
SWITCH_BATCHES = (1, 8, 256, 2048)
SWITCH_SETS = ((), ("KZ_FORCE_GENERIC",), ("KZ_NO_FUSED_HEADS",), ("KZ_NO_BOARD_CONV",), ("KZ_NO_RESIDENT_F16G",),
               ("KZ_KEEP_ACTIVATIONS",), ("KZ_FORCE_GENERIC", "KZ_KEEP_ACTIVATIONS"))
INDEX_CHARS = "".join(chr(c) for c in range(0x21, 0x7f) if chr(c) not in "\\\"")  # one JSON-safe character per entry
CHANNELS = (32, 48, 64, 96, 128, 160, 192, 256, 320, 384, 512)
LATTICE_GAMES = [  # (game, head): every board size the reference's server accepts a mapper for, with its usual head
    ("ataxx-4", "ataxx_conv"), ("ataxx-5", "ataxx_conv"), ("ataxx-6", "ataxx_conv"), ("ataxx-7", "ataxx_conv"),
    ("ataxx-8", "ataxx_conv"), ("chess", "attention"), ("chess-hist-1", "attention"), ("chess-hist-3", "attention"),
    ("chess", "dense"), ("go-9", "conv"), ("go-9-noterr", "conv"), ("go-13", "conv"), ("go-19", "conv"),
]


def plans(model):
    row = {}
    for arith in ("f32", "f16", "parity"):
        name = sweep_cases.parity_dtype_name(model, capi) if arith == "parity" else arith
        path, launches = model.plan(MAX_BATCH, DTYPES[name])
        row[arith] = {"dtype": name, "path": path, "launches": launches}
    return row


def build():
    paths = {}
    for case in sweep_cases.CASES:
        model = capi.Model(blob=synth.random_model(case.game, case.depth, case.channels, case.head, seed=11, **case.kw))
        paths[case.id] = {k: v["path"] for k, v in plans(model).items()}
    lattice = []
    for game, head in LATTICE_GAMES:
        g = synth.game_spec(game)
        for ch in CHANNELS:
            kw = dict(dense_hidden_channels=8) if head == "dense" else {}
            model = capi.Model(blob=synth.random_model(game, 2, ch, head, seed=1, **kw))
            lattice.append({"game": game, "squares": g["size"] ** 2, "c_in": g["n_scalar"] + g["n_bool"], "channels": ch,
                            "head": head, **plans(model)})
    return {"max_batch": MAX_BATCH, "paths": paths, "lattice": lattice, "switches": switches()}


def switches():
    """The selector under each switch set; the switches are read per call (kz_model_plan), so setting them in this
    process's environment is enough."""
    saved = {k: os.environ.pop(k) for k in {k for ks in SWITCH_SETS for k in ks} if k in os.environ}
    values, cases = [], {}
    try:
        for case in sweep_cases.CASES:
            model = capi.Model(blob=synth.random_model(case.game, case.depth, case.channels, case.head, seed=11, **case.kw))
            row = []
            for dtype in DTYPES.values():
                for mb in SWITCH_BATCHES:
                    for keys in SWITCH_SETS:
                        os.environ.update({k: "1" for k in keys})
                        try:
                            entry = "%s %d" % model.plan(mb, dtype)
                        except capi.KzError:
                            entry = "refused"
                        finally:
                            for k in keys:
                                del os.environ[k]
                        if entry not in values:
                            values.append(entry)
                        row.append(INDEX_CHARS[values.index(entry)])
            cases[case.id] = "".join(row)
    finally:
        os.environ.update(saved)
    return {"dtypes": list(DTYPES), "max_batch": list(SWITCH_BATCHES), "sets": [list(k) for k in SWITCH_SETS],
            "values": values, "cases": cases}


def build_bf16():
    """The bf16 column: every sweep case x max_batch (SWITCH_BATCHES) -> "path launches", or "refused"."""
    cases = {}
    for case in sweep_cases.CASES:
        model = capi.Model(blob=synth.random_model(case.game, case.depth, case.channels, case.head, seed=11, **case.kw))
        row = []
        for mb in SWITCH_BATCHES:
            try:
                row.append("%s %d" % model.plan(mb, capi.KZ_DTYPE_BF16))
            except capi.KzError:
                row.append("refused")
        assert (row[0] != "refused") == model.supports_dtype(capi.KZ_DTYPE_BF16), case.id
        cases[case.id] = row
    return {"max_batch": list(SWITCH_BATCHES), "cases": cases}


def build_int8(dtype=capi.KZ_DTYPE_INT8):
    """The int8 column: every sweep case, calibrated, x max_batch (SWITCH_BATCHES) -> "path launches", or "refused"; "no
    calibration" where the network cannot be calibrated at all."""
    cases, uncalibrated = {}, {}
    for case in sweep_cases.CASES:
        model = capi.Model(blob=synth.random_model(case.game, case.depth, case.channels, case.head, seed=11, **case.kw))
        assert not model.supports_dtype(dtype), case.id
        uncalibrated[case.id] = "refused"
        try:
            quant = model.quantize_int8([1.0] * len(model.range_sites()))
        except capi.KzError:
            cases[case.id] = ["no calibration"] * len(SWITCH_BATCHES)
            continue
        row = []
        for mb in SWITCH_BATCHES:
            try:
                row.append("%s %d" % quant.plan(mb, dtype))
            except capi.KzError:
                row.append("refused")
        assert (row[0] != "refused") == quant.supports_dtype(dtype), case.id
        cases[case.id] = row
    return {"max_batch": list(SWITCH_BATCHES), "cases": cases, "uncalibrated": uncalibrated}


def build_int8_heads():
    """The same column for dtype 5 (KZ_DTYPE_INT8_HEADS): the cases and batches of build_int8."""
    return build_int8(capi.KZ_DTYPE_INT8_HEADS)


def build_int8_any():
    """The same column for dtype 8 (KZ_DTYPE_INT8_ANY): the cases and batches of build_int8."""
    return build_int8(capi.KZ_DTYPE_INT8_ANY)


def markdown(table, rates, games=None):
    by = {}
    for r in rates:
        by.setdefault((r["squares"], r["c_in"], r["channels"], r["head"]), {})[r["arith"]] = r
    print("| board (squares) | input planes | channels | head | f32 | f16 | parity default |")
    print("|---|---|---|---|---|---|---|")
    for row in table["lattice"]:
        if games and row["game"] not in games:
            continue
        cells = []
        for arith in ("f32", "f16", "parity"):
            p = row[arith]
            txt = f"`{p['path']}` ({p['launches']})"
            m = by.get((row["squares"], row["c_in"], row["channels"], row["head"]), {}).get(arith)
            if m and "evals_per_s" in m and m.get("rate_path") == p["path"]:
                txt += f" **{m['evals_per_s'] / 1e3:,.0f}k** {m['frac_of_peak']:.2f} ({m.get('engines', 2)}e)"
            cells.append(txt)
        print(f"| {row['game']} ({row['squares']}) | {row['c_in']} | {row['channels']} | {row['head']} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--md", action="store_true")
    ap.add_argument("--rates", default=None)
    ap.add_argument("--games", default=None, help="comma-separated subset of the lattice's games for --md")
    ap.add_argument("--bf16", action="store_true", help="write the bf16 column (tests/golden/path_table_bf16.json)")
    ap.add_argument("--int8", action="store_true", help="write the int8 column (tests/golden/path_table_int8.json)")
    ap.add_argument("--int8-heads", action="store_true", help="write the dtype-5 column (tests/golden/path_table_int8_heads.json)")
    ap.add_argument("--int8-any", action="store_true", help="write the dtype-8 column (tests/golden/path_table_int8_any.json)")
    args = ap.parse_args()
    if args.int8_any:
        json.dump(build_int8_any(), open(OUT_INT8_ANY, "w"), indent=1, sort_keys=True)
        print("wrote", OUT_INT8_ANY)
    elif args.int8_heads:
        json.dump(build_int8_heads(), open(OUT_INT8_HEADS, "w"), indent=1, sort_keys=True)
        print("wrote", OUT_INT8_HEADS)
    elif args.int8:
        json.dump(build_int8(), open(OUT_INT8, "w"), indent=1, sort_keys=True)
        print("wrote", OUT_INT8)
    elif args.bf16:
        json.dump(build_bf16(), open(OUT_BF16, "w"), indent=1, sort_keys=True)
        print("wrote", OUT_BF16)
    elif args.md:
        rates = json.load(open(args.rates))["rows"] if args.rates else []
        markdown(json.load(open(OUT)), rates, args.games.split(",") if args.games else None)
    else:
        json.dump(build(), open(OUT, "w"), indent=1, sort_keys=True)
        print("wrote", OUT)
