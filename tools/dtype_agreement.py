"""Is this network inside the f16 contract on these positions?  The offline use of the shadow audit (kz_engine_set_audit,
DESIGN.md §6.4.4): an engine of --dtype with the audit at period 1 and boards = the batch, fed the positions of a position file
(kzero_amd/position_file.py: what self-play wrote, with the moves that were available) or synthetic boards, and the statistics the
engine accumulated beside the f16 contract README.md states for the decoded boundary (max |dp| <= 1e-3, rms 6e-4), with the
verdict inside / outside.  It reports and sets no bound of its own.

    python tools/dtype_agreement.py model.onnx|model.kzm [--scalars N] [--positions games_0 | --boards 1024] [--dtype f16]
                                    [--against split16|f32] [--batch 64] [--game chess]

--scalars: for ONNX, how many input planes are broadcast scalars (the mapper's input_scalar_count).  --positions: the path of a
position file without its extension.  --game: synthetic boards drawn like that game's (kzero_amd/synth.py) instead of uniformly.
--against defaults to split16 where the model has those kernels, else f32.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from kzero_amd import capi, synth  # noqa: E402
from kzero_amd.position_file import PositionFile  # noqa: E402

DTYPES = {"f16": capi.KZ_DTYPE_F16, "split16": capi.KZ_DTYPE_F32_SPLIT16, "f32": capi.KZ_DTYPE_F32}
CONTRACT_MAX_DP, CONTRACT_RMS = 1e-3, 6e-4  # README.md, the `KZ_HIP_DTYPE=f16` row
COLUMNS = ("value", "win", "draw", "loss", "moves_left")


def synthetic(info, n, game, seed=1):
    rng = np.random.default_rng(seed)
    if game:
        bits, scalars = synth.random_boards(game, n, seed=seed)
    else:
        nbits = info.input_bool_channels * info.board_h * info.board_w
        bits = np.packbits((rng.uniform(size=(n, nbits)) < 0.1).astype(np.uint8), axis=1, bitorder="little")
        scalars = rng.uniform(0, 1, size=(n, info.input_scalar_channels))
    moves = [rng.permutation(info.policy_len)[:int(k)].astype(np.int32) for k in rng.integers(1, min(info.policy_len, 61), size=n)]
    return np.ascontiguousarray(bits, np.uint8), np.ascontiguousarray(scalars, np.float32), moves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model")
    ap.add_argument("--scalars", type=int, help="ONNX: the number of scalar input planes")
    ap.add_argument("--positions", help="a position file (path without extension)")
    ap.add_argument("--boards", type=int, default=1024, help="synthetic boards when no position file is given")
    ap.add_argument("--game", help="draw the synthetic boards like this game's")
    ap.add_argument("--dtype", choices=("f16", "split16"), default="f16")
    ap.add_argument("--against", choices=("split16", "f32"))
    ap.add_argument("--batch", type=int, default=64, help="at most 64: the sibling engine's max_batch")
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the table")
    args = ap.parse_args()
    assert capi.device_count() >= 1, "needs a GPU"
    assert 1 <= args.batch <= 64, "--batch must be in 1..64 (the audit's sibling engine holds at most 64 boards)"

    model = capi.Model(path=args.model, onnx_scalar_channels=args.scalars)
    info = model.info
    against = args.against or ("split16" if args.dtype != "split16" and model.supports_dtype(capi.KZ_DTYPE_F32_SPLIT16) else "f32")
    if args.positions:
        bits, scalars, moves = PositionFile(args.positions).read_boards()
        source = f"{len(moves)} positions of {args.positions}"
    else:
        bits, scalars, moves = synthetic(info, args.boards, args.game)
        source = f"{len(moves)} synthetic boards" + (f" ({args.game})" if args.game else "")
    eng = capi.Engine(model, 0, args.batch, DTYPES[args.dtype])
    eng.set_audit(DTYPES[against], 1, args.batch)
    bad = 0
    for lo in range(0, len(moves), args.batch):
        hi = min(lo + args.batch, len(moves))
        _, _, status = eng.eval_packed_decoded_status(bits[lo:hi], scalars[lo:hi], moves[lo:hi])
        bad += int((status != capi.KZ_BOARD_OK).sum())
    st = eng.audit_stats()
    inside = bool(st.boards > 0 and st.max_abs_prob <= CONTRACT_MAX_DP and st.rms_prob <= CONTRACT_RMS)
    if args.json:
        print(json.dumps({"tool": "dtype_agreement", "model": args.model, "tower_path": eng.tower_path, "dtype": args.dtype,
                          "against": against, "source": source, "boards": st.boards, "moves": st.moves, "skipped": st.skipped,
                          "max_abs_prob": float(st.max_abs_prob), "rms_prob": st.rms_prob,
                          "max_abs_value": dict(zip(COLUMNS, map(float, st.max_abs_value))),
                          "rms_value": dict(zip(COLUMNS, map(float, st.rms_value))),
                          "contract": {"max_abs_prob": CONTRACT_MAX_DP, "rms": CONTRACT_RMS}, "inside": inside}))
        return
    print(f"{args.model}: {args.dtype} ({eng.tower_path}) against {against}, {source}")
    print(f"  compared {st.boards} boards, {st.moves} probabilities; skipped {st.skipped} (status not 0 on either side; {bad} in the {args.dtype} engine)")
    print(f"  {'':12s}{'max |d|':>12s}{'rms':>12s}{'f16 contract':>28s}")
    print(f"  {'probability':12s}{float(st.max_abs_prob):12.3e}{st.rms_prob:12.3e}{f'max <= {CONTRACT_MAX_DP:g}, rms <= {CONTRACT_RMS:g}':>28s}")
    for c, name in enumerate(COLUMNS):
        print(f"  {name:12s}{float(st.max_abs_value[c]):12.3e}{float(st.rms_value[c]):12.3e}")
    print(f"  -> {'inside' if inside else 'outside'} the f16 contract on these positions" if st.boards else "  -> nothing was compared")


if __name__ == "__main__":
    main()
