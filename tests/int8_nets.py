"""Networks for the int8 tower (KZ_DTYPE_INT8, kz_tower_i8.hip), on the draws of tests/exact_nets.py: a float64 reference that
quantises where the launch quantises (`int8_reference`, written from the arithmetic of include/kz_hip.h, "int8 calibration"),
and two families it decides to the bit.  Integer dot products are exact and every scale is a power of two, so what a site
rounds is one f32 value in any summation order: there is no tolerance.  Test infrastructure only, no GPU.

  exact family     the narrow networks of exact_nets (no dense layer): every quantised tensor and every tower weight an integer
                   within +-127 at exponent 0 (calibration maximum 127 at every site).  Nothing rounds, nothing clamps: the int8
                   reference equals the unquantised float64 reference bit for bit, `sums` as in exact_nets.
  rounding family  values that do not fit.  From the same draws, optionally with one dense tower layer (asymmetric weights on
                   every lane of every fragment), the biases changed by channel class (c % 8, `CLASSES`) so that every quantised
                   site meets ties in both directions, values that are no tie and values beyond +-127 steps, and the stem's
                   output — the one site in front of a ReLU — values below -127 steps.  The calibration maxima are chosen from
                   the unquantised reference (`calibration`), never from the launch, and include the last site's (accepted and ignored).  The heads read the integer classes only:
                   behind the tower every value is a short dyadic number again, so the f16 head kernels stay exact and the
                   tower alone decides the bits (`head_conditions`).
  ... with weights that round (`build_round(..., weights="round")`, WEIGHT_NETS): both families draw weights of +-1 and +-2,
                   which are +-32 or +-64 steps of their row: `wq = rne(w 2^-f)` has nothing to round and only two bits of a
                   weight byte ever differ.  This variant gives every row of every conv A entries that are ties in both
                   directions and non-ties at that row's own step, and some rows a top of 127 steps (`_round_weights`).  The
                   weights stay short dyadic numbers, the reference rounds them as it rounds any.

The networks (`NETS`) are chosen by what the launch does with their shape — boards per workgroup, idle rows, stem chunks,
widened towers, depth —, not by game; the table says which is there for what.

The report counts, per quantised site, ties that go down, ties that go up, non-ties, clamps at +127 and clamps at -127
(tests/test_int8_nets.py holds floors on them), and `mutants` lists references that quantise otherwise.
"""
import numpy as np

from tests import exact_nets as E

QMAX = 127.0
# channel classes of the rounding family, by c % 8: what the biases of that channel carry
#   0, 3, 4  integers, as drawn: the only channels the heads read
#   1        the stem's bias and conv A's + 1/2: exact ties at an even exponent <= 0, both directions by the parity of the integer part
#   2        ... + 1/4: no tie
#   5        the stem's bias - BIG: below -127 steps at site 0 (behind a ReLU nothing is negative)
#   6        every bias + BIG: beyond +127 steps at every site
#   7        the stem's bias and conv A's + 1/2 + 2^-9 on a magnitude >= 8: no tie in f32, a tie once rounded to f16 — what tells
#            X8 = quant(v) from X8 = quant(f16(v))
HEAD_CLASSES = (0, 3, 4)
FRACTION = {1: 0.5, 2: 0.25, 7: 0.5 + 2.0 ** -9}
BIG = 160.0
F16_LIFT = 12.0  # class 7: the integer part of the bias, so that |v| >= 8 and f16 drops the 2^-9


def i8_exponent(m):
    """ceil(log2(m / 127)) from the definition: the smallest e with 127 * 2^e >= m, in exact arithmetic."""
    m = float(m)
    assert np.isfinite(m) and m > 0
    e = int(np.floor(np.log2(m))) - 8
    while 127.0 * 2.0 ** e < m:
        e += 1
    return e


def _round(s, mode):
    if mode == "trunc":
        return np.trunc(s)
    if mode == "half-away":
        return np.sign(s) * np.floor(np.abs(s) + 0.5)
    return np.rint(s)  # to nearest, ties to even


def quant(v, e, mode="rne", lo=-QMAX):
    """clamp(round(v * 2^-e), lo, 127): the int8 image, as float64 integers."""
    return np.clip(_round(np.asarray(v, np.float64) * 2.0 ** -e, mode), lo, QMAX)


def f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def f16(v):
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def folded(t, meta):
    """[(w, b)] of the 1 + 2 depth tower convolutions with their BatchNorm folded (W' = s W, b' = s (b - mean) + beta), and the
    final BN as (scale, shift); float64.  The families' BatchNorms have s = 1: the fold is exact, asserted."""
    eps, depth = meta["bn_eps"], meta["tower_depth"]

    def bn(p):
        s = 1.0 / np.sqrt(t[p + ".running_var"].astype(np.float64) + eps)
        g = t[p + ".weight"].astype(np.float64) if p + ".weight" in t else 1.0
        b = t[p + ".bias"].astype(np.float64) if p + ".bias" in t else 0.0
        return s * g, b - t[p + ".running_mean"].astype(np.float64) * s * g
    out = [(t["common.tower.0.weight"].astype(np.float64), t["common.tower.0.bias"].astype(np.float64))]
    for i in range(1, depth + 1):
        for c, n in ((0, 1), (3, 4)):
            p = f"common.tower.{i}.seq."
            s, sh = bn(p + str(n))
            w = t[p + f"{c}.weight"].astype(np.float64) * s[:, None, None, None]
            b = t[p + f"{c}.bias"].astype(np.float64) * s + sh
            assert E.f32_exact(w) and E.f32_exact(b), "the fold must be exact in f32"
            out.append((w, b))
    return out, bn(f"common.tower.{depth + 1}")


def weight_steps(w):
    """(w 2^-f, f): a block convolution's weights in steps of their output channel, f = ceil(log2(max |w[oc]| / 127)); an
    all-zero filter has f = 0."""
    top = np.abs(w).reshape(w.shape[0], -1).max(axis=1)
    f = np.array([i8_exponent(m) if m > 0 else 0 for m in top])
    return w * 2.0 ** -f.astype(np.float64)[:, None, None, None], f


def quantise_weights(w, mode="rne"):
    """(wq, f): per output channel f as in `weight_steps`, wq = rne(w 2^-f) (mode: another `_round`, for the weight mutants)."""
    s, f = weight_steps(w)
    return _round(s, mode), f


def _tie_counts(s):
    """(ties that go down, ties that go up, non-ties) of round-to-nearest-even on s, by magnitude."""
    frac = np.abs(s) - np.floor(np.abs(s))
    tie = frac == 0.5
    even = np.floor(np.abs(s)) % 2 == 0
    return int((tie & even).sum()), int((tie & ~even).sum()), int(((frac != 0) & ~tie).sum())


class Report:
    def __init__(self):
        self.counts = {}   # quantised site -> (ties down, ties up, non-ties, clamps at +127, clamps at -127, values)
        self.exact = {}    # step -> every f32 rounding of the launch had nothing to round (the reference's own condition)
        self.acc_max = 0   # largest |acc|
        self.sites = {}    # site -> what was stored (X8 / Y8 as integers; the stream as f16 values under "<site>.x")
        self.wq_max = 0
        self.wcounts = {}  # block convolution (1 .. 2 depth) -> (weight ties down, ties up, non-ties) of wq = rne(w 2^-f)
        self.wq = {}       # block convolution -> the sorted values wq takes

    def count(self, name, v, e):
        s = np.asarray(v, np.float64) * 2.0 ** -e
        r = np.rint(s)
        self.counts[name] = _tie_counts(s) + (int((r > QMAX).sum()), int((r < -QMAX).sum()), int(s.size))


def int8_tower(t, meta, x, exps, mutant=None):
    """The tower output (behind the final BN, as the f16 rows that leave the launch) and the report.  exps: e_s of the
    2 depth quantised sites (a mutant that quantises the last site too takes one more).  mutant: None, or
      ("round", mode)     mode "trunc" / "half-away" in place of nearest-even at every site
      ("clamp128",)       the lower clamp at -128
      ("from-f16",)       X8 quantised from f16(v) instead of v
      ("residual-first",) the residual added before the ReLU
      ("more",)           the last site quantised too (and carried on at its step)
      ("without", s)      site s not quantised: its values in steps, unrounded and unclamped, go into the convolution
      ("weights", mode)   the weights rounded by mode "trunc" / "half-away" in place of nearest-even (the sites as they are)"""
    depth = meta["tower_depth"]
    layers, (ps, pt) = folded(t, meta)
    rep = Report()
    kind = mutant[0] if mutant else None
    mode = mutant[1] if kind == "round" else "rne"
    wmode = mutant[1] if kind == "weights" else "rne"
    lo = -128.0 if kind == "clamp128" else -QMAX
    names = ["tower.0"] + [n for i in range(1, depth + 1) for n in (f"tower.{i}.mid", f"tower.{i}")]

    def q(site, v, src=None):
        e = exps[site]
        rep.count(names[site], v, e)
        if kind == "without" and mutant[1] == site:
            out = np.asarray(v, np.float64) * 2.0 ** -e
        else:
            out = quant(v if src is None else src, e, mode, lo)
        rep.sites[names[site]] = out
        return out

    def checked_f32(step, v):
        r = f32(v)
        rep.exact[step] = rep.exact.get(step, True) and bool(np.array_equal(r, v))
        return r

    def conv(l, img, e_in):
        w, b = layers[l]
        wq, f = quantise_weights(w, wmode)
        rep.wq_max = max(rep.wq_max, float(np.abs(wq).max()))
        rep.wcounts[l] = _tie_counts(weight_steps(w)[0])
        rep.wq[l] = np.unique(wq)
        acc = E._lin(img, wq, mags=False)[0]  # exact: integers below 2^53
        rep.acc_max = max(rep.acc_max, float(np.abs(acc).max()))
        tt = f32(acc)  # v_cvt_f32_i32, nearest even
        mult = 2.0 ** (e_in + f.astype(np.float64))
        return checked_f32(f"layer{l}.bias", tt * mult[None, :, None, None] + b[None, :, None, None])

    # the stem in f16 operands, f32 accumulation: exact on these families (asserted through `exact`)
    w0, b0 = layers[0]
    assert np.array_equal(f16(w0), w0) and np.array_equal(f16(x), x), "the stem's operands are f16 values"
    v = checked_f32("stem", E._lin(np.asarray(x, np.float64), w0, mags=False)[0] + b0[None, :, None, None])
    xs = f16(v)
    x8 = q(0, v, xs if kind == "from-f16" else None)
    rep.sites["tower.0.x"] = xs
    out = None
    for i in range(1, depth + 1):
        a, bl = 2 * i - 1, 2 * i
        v = np.maximum(conv(a, x8, exps[a - 1]), 0.0)
        y8 = q(a, v)
        v = conv(bl, y8, exps[a])
        if kind == "residual-first":
            v = np.maximum(checked_f32(f"layer{bl}.residual", v + xs), 0.0)
        else:
            v = checked_f32(f"layer{bl}.residual", np.maximum(v, 0.0) + xs)  # added in f32, AFTER the ReLU
        if i < depth:
            xs = f16(v)
            x8 = q(bl, v, xs if kind == "from-f16" else None)
            rep.sites[f"tower.{i}.x"] = xs
        else:
            if kind == "more":
                v = quant(v, exps[bl], mode, lo) * 2.0 ** exps[bl]
            out = f16(checked_f32("final_bn", v * ps[None, :, None, None] + pt[None, :, None, None]))
    return out, rep


def int8_reference(t, meta, x, exps, mutant=None, exact=True):
    """(scalars [B, 5], policy [B, P], tower report, heads report): the int8 tower, then exact_nets' heads on its output."""
    common, rep = int8_tower(t, meta, x, exps, mutant)
    site = f"tower.{meta['tower_depth'] + 1}"
    s, p, heads = E.reference(t, meta, x, exact=exact, rounding=(frozenset({site}), lambda v: common))
    return s, p, rep, heads


def head_conditions(heads, depth):
    """The f16 head kernels return the float64 bits: every tensor they read or store (the tower output, the hidden layers, the
    heads' weights) is an f16 value, every sum of theirs within SUM_MAX steps, and the outputs are exact in f32 (asserted by
    the reference itself)."""
    ok = all(v <= E.SUM_MAX for k, v in heads.sums.items() if not k.startswith("common."))
    for k, v in heads.values.items():
        if k.startswith(("scalar_head", "policy_head")) or k == f"tower.{depth + 1}":
            ok = ok and bool(np.array_equal(f16(v), v))
    return ok


# ---- the two families ----
# the networks of tests/test_gpu_int8_exact.py: (game, depth, channels, head, keywords)
NETS = {
    "chess_2x256_att": ("chess", 2, 256, "attention", {}),   # 256 channels, the attention head outside
    "chess_1x256_att": ("chess", 1, 256, "attention", {}),   # depth 1: the last-layer epilogue alone
    "chesshist1_1x256_att": ("chess-hist-1", 1, 256, "attention", {}),  # 34 input planes: two stem chunks
    "chess_2x128_att": ("chess", 2, 128, "attention", dict(query_channels=64)),  # 128 channels in four tiles (1 / sqrt(64) is a power of two)
    "ataxx7_2x128": ("ataxx-7", 2, 128, "ataxx_conv", {}),   # two boards in seven tiles
    "go9_3x128": ("go-9", 3, 128, "conv", {}),               # one board in six tiles, two block boundaries
    # ---- the geometries the plan accepts beside those: the instance is chosen by tile count, nb = floor(16 NT / hw) boards per
    # workgroup, 112 rows at 128 channels (any board of at most 56 squares) and 64 at 256 ----
    "ttt_2x128_dense": ("ttt", 2, 128, "dense", {}),         # 3x3: 12 boards in seven tiles
    "ataxx4_2x128": ("ataxx-4", 2, 128, "ataxx_conv", {}),   # 7 boards, every board edge on a tile edge
    "ataxx5_2x128": ("ataxx-5", 2, 128, "ataxx_conv", {}),   # 4 boards
    "ataxx6_2x128": ("ataxx-6", 2, 128, "ataxx_conv", {}),   # 3 boards
    "ataxx7_2x96": ("ataxx-7", 2, 96, "ataxx_conv", {}),     # widened to 128 (all-zero filters, f = 0), two boards in seven tiles
    "arimaa_2x96": ("arimaa-split", 2, 96, "arimaa", {}),    # widened, 38 input planes: two stem chunks at 128 channels
    "chess_4x128_att": ("chess", 4, 128, "attention", dict(query_channels=64)),  # three block boundaries: the ring, g, fetch_tables
    "ataxx4_2x256": ("ataxx-4", 2, 256, "ataxx_conv", {}),   # 4 boards in four tiles, no idle row
    "ataxx5_2x256": ("ataxx-5", 2, 256, "ataxx_conv", {}),   # 2 boards, 14 idle rows
    "ataxx6_2x256": ("ataxx-6", 2, 256, "ataxx_conv", {}),   # one board, 28 idle rows
    "ataxx7_2x256": ("ataxx-7", 2, 256, "ataxx_conv", {}),   # one board, 15 idle rows
    "chess_2x200_att": ("chess", 2, 200, "attention", dict(query_channels=64)),  # widened to 256, and the two-board launch
    "chesshist4_1x256_att": ("chess-hist-4", 1, 256, "attention", {}),  # 73 input planes: three stem chunks, stem rows of 128 B
    "chesshist7_1x256_att": ("chess-hist-7", 1, 256, "attention", {}),  # 112 input planes: four stem chunks
    "ataxx2_2x128": ("ataxx-2", 2, 128, "ataxx_conv", {}),   # 2x2: every square a corner, 28 boards
    "ataxx2_2x256": ("ataxx-2", 2, 256, "ataxx_conv", {}),   # ... 16 boards
    "ttt_2x256_dense": ("ttt", 2, 256, "dense", {}),         # 3x3 at 256 channels: 7 boards, one idle row
}
# A network may be in the rounding family only if every mutant of `mutants` returns other outputs on it: a rounding case must
# tell each of them from the launch (tests/test_int8_nets.py holds that on every network of ROUND_NETS).  With the common seed
# four networks lose "clamp-128" (arimaa_2x96, ttt_2x256_dense) or "clamp-128" and "from-f16" (ataxx-2 at both widths): no value
# below -127.5 steps at the stem's site reaches a channel the heads read.  A seed of their own repairs all four (ROUND_SEED: the first of
# 2, 3, ... with no such mutant), so every network is in both families and EXACT_ONLY, where one that cannot be repaired goes,
# is empty.
EXACT_ONLY = set()
ROUND_NETS = [n for n in NETS if n not in EXACT_ONLY]
# the rounding family with weights that round (`build_round`, weights="round"): one network per instance of the kernel's table
WEIGHT_NETS = ["chess_2x256_att", "chess_2x128_att", "ataxx7_2x128", "go9_3x128"]
ALL_DENSE = ("chess_2x256_att", "chess_1x256_att", "chesshist1_1x256_att", "chess_2x128_att", "ataxx7_2x128", "go9_3x128")
SEED = E.SEED
ROUND_SEED = {"arimaa_2x96": 2, "ataxx2_2x128": 5, "ataxx2_2x256": 2, "ttt_2x256_dense": 2}  # rounding family: network and boards drawn from this seed
BOARDS = E.BOARDS


def widened(channels):
    """The tower width the int8 plan runs a network at: 65 .. 128 channels as 128, 193 .. 256 as 256."""
    return 128 if channels <= 128 else 256


def boards_per_workgroup(channels, hw):
    """At max_batch 64, by the rule of the instance table (kz_tower_i8.hip): the tile count follows from the (widened) channels
    and the board — 64 rows at 256 channels; at 128 channels 112 for a board of at most 56 squares, else 64, else 96 —, and a
    workgroup takes as many whole boards as its rows hold."""
    if widened(channels) == 256:
        rows = 64
    else:
        rows = 112 if hw <= 56 else 64 if hw <= 64 else 96
    return rows // hw


def dense_positions(net):
    """None and the block convolutions that take the dense layer (layer_names order: 1 .. 2 depth): every one on the six
    networks of ALL_DENSE — between them every lane of every instance's weight fragments —, the first conv A and the last
    conv B on the others, which are there for their geometry."""
    depth = NETS[net][1]
    return [None] + (list(range(1, 2 * depth + 1)) if net in ALL_DENSE else [1, 2 * depth])


class Built:
    pass


_CACHE = {}


def _finish(b, t, meta, bits, scalars, site_max):
    b.meta, b.tensors, b.bits, b.scalars_in = meta, t, bits, scalars
    b.x = E.encode(meta, bits, scalars)
    b.site_max = np.asarray(site_max, np.float32)
    b.exps = [i8_exponent(m) for m in b.site_max]
    s, p, b.report, b.heads = int8_reference(t, meta, b.x, b.exps)
    b.ref_scalars, b.ref_policy = s.astype(np.float32), p.astype(np.float32)
    b.blob = E.write_model(meta, t)
    return b


EXACT_ENTRIES = 12  # exact family, dense_at: that block convolution has about this many weights per output row, anywhere


def build_exact(net, dense_at=None):
    """A network of exact_nets — narrow, or with block convolution `dense_at` drawn from DENSE_VALUES at EXACT_ENTRIES weights
    per row: asymmetric integers spread over every lane of the weight fragments — with the calibration maximum 127 steps at every
    site, a step being 1 (chess) or 1/2 (Ataxx and Go have scalar planes in halves): nothing rounds, nothing clamps."""
    key = ("exact", net, dense_at)
    if key not in _CACHE:
        while len(_CACHE) >= 12:
            _CACHE.pop(next(iter(_CACHE)))
        game, depth, channels, head, kw = NETS[net]
        bits, scalars = E.exact_boards(game, BOARDS, SEED)
        meta, t, seed, (s, p, rep) = E.draw_exact(game, depth, channels, head, dense_at, SEED, boards=(bits, scalars),
                                                  density=EXACT_ENTRIES / (9.0 * channels), **kw)
        step = min(E.step_of(v) for k, v in rep.acts.items() if k.startswith("tower.") and v.ndim == 4)
        b = _finish(Built(), t, meta, bits, scalars, [QMAX * min(step, 1.0)] * (2 * depth + 1))
        b.dense_at, b.step = dense_at, step
        b.plain_scalars, b.plain_policy, b.plain_report = s.astype(np.float32), p.astype(np.float32), rep
        _CACHE[key] = b
    return _CACHE[key]


def _classes(t, meta):
    """The rounding family's biases by channel class (module docstring), and heads that read the integer classes only."""
    depth, C = meta["tower_depth"], meta["tower_channels"]
    cls = np.arange(C) % 8
    frac = np.zeros(C)
    for k, f in FRACTION.items():
        frac[cls == k] = f
    b0 = t["common.tower.0.bias"].astype(np.float64)
    b0 = b0 + frac + np.where(cls == 7, F16_LIFT, 0.0) + np.where(cls == 6, BIG, 0.0) - np.where(cls == 5, BIG, 0.0)
    t["common.tower.0.bias"] = b0.astype(np.float32)
    for i in range(1, depth + 1):
        ka, kb = f"common.tower.{i}.seq.1.bias", f"common.tower.{i}.seq.4.bias"
        t[ka] = (t[ka].astype(np.float64) + frac + np.where(cls == 7, F16_LIFT, 0.0) + np.where(cls == 6, BIG, 0.0)).astype(np.float32)
        t[kb] = (t[kb].astype(np.float64) + np.where(cls == 6, BIG, 0.0)).astype(np.float32)
    for p in E._HEAD_FIRST:
        if p + ".weight" in t:
            t[p + ".weight"][:, ~np.isin(cls, HEAD_CLASSES)] = 0.0


def calibration(t, meta, x):
    """Calibration maxima from the UNQUANTISED float64 reference: per site the 0.7 quantile of the non-zero magnitudes (the
    +-BIG classes, a quarter of the channels, lie above it and clamp; tests/test_int8_nets.py holds the clamped share below a
    half), at least 127: a site of small values has exponent 0, where the
    class biases are ties and near-ties; behind a dense layer the exponent is what the values ask for."""
    _, _, rep = E.reference(t, meta, x, exact=False, rounding=(frozenset(), None))
    depth = meta["tower_depth"]
    names = ["tower.0"] + [n for i in range(1, depth + 1) for n in (f"tower.{i}.mid", f"tower.{i}")]
    names[-1] = f"tower.{depth + 1}"
    out = []
    for n in names:
        v = np.abs(rep.values[n])
        v = v[v > 0]
        out.append(max(float(np.quantile(v, 0.7)) if v.size else 1.0, QMAX))
    return out


# weights="round": what every output row of conv A that has a weight gets more, in steps of THAT row — its drawn top is a
# power of two, 64 steps (top 1: f = -6, a step 1/64; a dense row with a +-2: f = -5) —: ties that go down (1/2, 2 1/2) and
# up (-1 1/2, 3 1/2) and values that are no tie (-3/4, 1/4), of both signs ...
WEIGHT_EXTRA = (0.5, -1.5, 2.5, -0.75, 3.5, 0.25)
# ... and one such row in TOP_EVERY has its first entry at 127 of those steps, its sign the entry's: f stays what it was, wq
# takes -127 and +127 and, with the extras on that row, odd values between — every bit of a weight byte is used
WEIGHT_TOP, TOP_EVERY = 127.0, 4


def _round_weights(t, meta, seed):
    """The weight-rounding variant, in conv A of every block and only there: conv A's output goes to Y8 alone, quantised before
    anything else reads it, while fractions in conv B would reach the unquantised f16 stream and the heads.  The weights stay
    short dyadic numbers: `quantise_weights` rounds them as it rounds any.  A row without a weight stays all-zero (f = 0)."""
    for i in range(1, meta["tower_depth"] + 1):
        rng = np.random.default_rng([seed, 86028121, i])
        w = t[f"common.tower.{i}.seq.0.weight"]
        w2 = w.reshape(w.shape[0], -1)  # (a view)
        for r in range(w2.shape[0]):
            top = float(np.abs(w2[r]).max())
            if top == 0:
                continue
            assert np.log2(top) == np.round(np.log2(top)), "the drawn top of a row is a power of two: 64 steps"
            step = top / 64.0
            if r % TOP_EVERY == 1:
                j = int(np.flatnonzero(w2[r])[0])
                w2[r, j] = np.float32(np.sign(w2[r, j]) * WEIGHT_TOP * step)
            free = np.flatnonzero(w2[r] == 0)
            w2[r, rng.choice(free, size=len(WEIGHT_EXTRA), replace=False)] = (np.array(WEIGHT_EXTRA) * step).astype(np.float32)


def build_round(net, dense_at, weights=None):
    """A network of the rounding family: exact_nets' draw (dense_at: that block convolution dense), the class biases, the
    calibration of `calibration`.  weights="round": conv A's weights round too (`_round_weights`)."""
    key = ("round", net, dense_at, weights)
    if key not in _CACHE:
        while len(_CACHE) >= 12:
            _CACHE.pop(next(iter(_CACHE)))
        game, depth, channels, head, kw = NETS[net]
        seed = ROUND_SEED.get(net, SEED)
        bits, scalars = E.exact_boards(game, BOARDS, seed)
        meta, t = E._draw(game, depth, channels, head, dense_at, seed, 1.0, kw)
        _classes(t, meta)
        if weights == "round":
            _round_weights(t, meta, seed)
        else:
            assert weights is None
        x = E.encode(meta, bits, scalars)
        b = _finish(Built(), t, meta, bits, scalars, calibration(t, meta, x))
        b.dense_at, b.weights = dense_at, weights
        _CACHE[key] = b
    return _CACHE[key]


def mutants(b):
    """{name: mutant} of every reference that quantises otherwise than the launch is said to (the weight mutants where the
    weights round: elsewhere every weight is an integer number of steps and they are the reference itself)."""
    depth = b.meta["tower_depth"]
    m = {"truncate": ("round", "trunc"), "half-away": ("round", "half-away"), "clamp-128": ("clamp128",), "from-f16": ("from-f16",),
         "residual-first": ("residual-first",), "one-site-more": ("more",)}
    for s in range(2 * depth):
        m[f"without-{s}"] = ("without", s)
    if getattr(b, "weights", None) == "round":
        m["weights-truncate"] = ("weights", "trunc")
        m["weights-half-away"] = ("weights", "half-away")
    return m


def run_mutant(b, mutant):
    s, p, _, _ = int8_reference(b.tensors, b.meta, b.x, b.exps, mutant, exact=False)
    return s.astype(np.float32), p.astype(np.float32)
