"""Exactly representable networks: every weight, bias, input and stored intermediate a short dyadic number, every partial
sum within 24 bits.  On such a network f32, f16 and split arithmetic (lo halves zero) all return the bits a float64
evaluation returns, in any summation order: a difference is an indexing, padding, packing or batching error, never
rounding (DESIGN.md "Exact networks").  Test infrastructure only, no GPU.

`exact_model` draws the network, `exact_boards` the positions, `reference` is PredictionHeads.forward
(python/lib/model/post_act.py:187-228 with ScalarHead :10-23 and the policy heads :26-173) in plain numpy float64,
written from that definition and sharing nothing with oracle/kz_oracle.c.  It also measures the two conditions:

  stored:  every tensor a kernel may keep in f16 round-trips through np.float16 and has max |v| / step <= 1024, step the
           largest power of two dividing all its values (half of what f16 holds: a kernel that stores one more
           intermediate, or a (hi, lo) pair, stays exact);
  sums:    every accumulation has sum |a b| / step <= 2^22: exact in f32 whatever the order of the additions and however
           the matrix unit aligns its 32 products, as long as it keeps 24 bits.

On those networks a split16 engine's lo halves are all zero.  The wide family (`wide=` of `draw_exact` / `build`, from the
same draws: `_widen`) has weights, scalar planes and activations that need a (hi, lo) pair, and holds in place of `stored`:

  split-stored:  every such tensor and every layer's weights satisfy v == hi + lo with lo = f16(v - hi), for hi either
                 f16 neighbour of v, |v| <= 32752, no non-zero lo below 2^-14 (`split_exact`);
  no lo.lo:      of the two operands of every product a split kernel forms one has no lo half at all, and
                 hi*hi + hi*lo + lo*hi, computed a second time in float64, equals the plain result;

`sums` as above with the step of the wide values.  The report also says where the lo halves are (`lo_in`, `lo_w`):
tests/test_exact_nets.py holds that every layer meets them in its input and in every weight fragment.

The rounding family (`draw_rounding` / `build_round`, `rounding=` of `reference`) is for a launch that rounds on purpose: the
bf16 tower keeps its images and weights in 8 significant bits.  Its values do NOT fit the stored format, and the reference
rounds where the launch rounds (`bf16_sites`, read off kz_tower_pairs.hpp), by `bf16_rne`.  What a site rounds is one f32
value, the same in any summation order, so the result is still a matter of bits.  In place of `stored`:

  rounded:  every value in front of a rounding and every stored tensor is finite and exact in f32 (the launch forms it in
            f32: accumulator, ReLU, residual add, final BN), and the outputs are exact in f32;

`sums` as above, with the steps of the rounded operands.  The report counts, per site, the ties that go down, the ties that
go up and the values that are no tie: tests/test_round_nets.py holds floors on them and shows that references which round
otherwise, elsewhere, once more or once less return other outputs.

The scaled family (`build_scaled`) is a narrow network with the layers that write its outputs times powers of two: still
exact, logits of any spread.  With `decode_ref`, a float64 decode_output, it is the reference of the launches' decode
(tests/decode_cases.py, tests/test_decode_nets.py, tests/test_gpu_decode_exact.py).
"""
import numpy as np

from kzero_amd import synth
from kzero_amd.model_file import read_model, write_model

STORED_MAX = 1024
SUM_MAX = 1 << 22
BN_EPS = 2.0 ** -17          # running_var = 1 - 2^-17 is exact in f32, and var + eps == 1.0: Conv+BN folds without rounding
DENSE_VALUES = (-2.0, -1.0, 1.0, 2.0)  # magnitudes as well as signs: a permutation inside one sign class shows too
# one weight in sixteen has magnitude 2: drawn evenly, a dense 256-channel layer in front of the attention head takes
# sum |q_from q_to| past 2^22 (measured 5.7e6 and 6.3e6 on chess 2x256, 4.6e6 with one in eight; 256 terms of |q|^2, |q| ~ 48 * rms(w) * rms(x))
DENSE_P = (1 / 32, 15 / 32, 15 / 32, 1 / 32)
SPARSE_PER_ROW = 2
LIVE_SHARE = 0.25            # every channel behind a ReLU is positive on at least this share of the (board, square) positions
HEAD_SCALE = 0.25            # first layer of every head branch: power-of-two scaling costs no bits and keeps the sums small
# ---- the wide family (module docstring, "wide") ----
WIDE = 1.0 + 2.0 ** -11      # +-1 and +-1/4 times this: hi = the weight, lo = 2^-11 of it, both exact in f16 whichever neighbour is hi
SPLIT_MAX = 32752.0          # half of f16's range
LO_MIN = 2.0 ** -14          # f16's smallest normal number: no non-zero lo half below it
FRAGMENT_ENTRIES = 3         # wide weights drawn per weight fragment: one reads one channel on one tap, which a board may leave empty
LANE = 4                     # attention networks: channel c with c % LANE == LANE - 1 reads such channels only and stays narrow
NARROW_Q, NARROW_ON = 16, 128
# ... and the narrow operand of q_from . q_to reads the tower on NARROW_Q query channels, is a constant +-1/4 (its bias alone: one
# step) on more, NARROW_ON in all, and zero on the rest, each evenly spaced.  A wide value is >= 2^11 steps by definition and
# the tower's output a few units, so 256 query channels at one step each already come to 2^22 (measured on chess 2x256, all
# 256 on: 8.0e6 to 1.0e7 with every one reading the tower, 2.6e6 to 4.7e6 with 32 of them; as committed 2.3e6 at the most);
# Q = 64 keeps every channel on.


def layer_names(tensors):
    """Convolution and linear layers in execution order (the state_dict's order): stem, tower convolutions, heads."""
    return [k[:-len(".weight")] for k, v in tensors.items()
            if k.endswith(".weight") and v.ndim in (2, 4) and k[:-len(".weight")] + ".running_mean" not in tensors]


# the attention head multiplies two of its convolutions' outputs: one entry per row keeps sum |q_from q_to| within 2^22
_ONE_PER_ROW = {"policy_head.conv_bulk": 1, "policy_head.conv_under": 1}
_HEAD_FIRST = ("scalar_head.seq.0", "policy_head.seq.0", "policy_head.seq_extra.0", "policy_head.conv_bulk",
               "policy_head.conv_under", "policy_head.bulk.0", "policy_head.scalar.0")


def _draw(game, depth, channels, head, dense_at, seed, density, kw, wide=None):
    meta, t0 = read_model(synth.random_model(game, depth, channels, head, seed=seed, **kw))
    rng = np.random.default_rng([seed, 7919, 0 if dense_at is None else 1 + dense_at])
    t = {k: v.copy() for k, v in t0.items()}
    meta["bn_eps"] = BN_EPS
    names = layer_names(t)
    if dense_at is not None and not 0 <= dense_at < len(names):
        raise IndexError(f"dense_at {dense_at}: the network has {len(names)} layers")
    for k in list(t):
        if k.endswith(".running_mean"):
            p = k[:-len(".running_mean")]
            c = t[k].shape[0]
            t[p + ".running_mean"] = np.zeros(c, np.float32)
            t[p + ".running_var"] = np.full(c, 1.0 - BN_EPS, np.float32)
            if p + ".weight" in t:  # (final_affine=False: no weight / bias)
                t[p + ".weight"] = np.ones(c, np.float32)
                t[p + ".bias"] = _bias(rng, c)
    for i, p in enumerate(names):
        shape = t[p + ".weight"].shape
        rows, fan = shape[0], int(np.prod(shape[1:]))
        if i == dense_at:
            w = rng.choice(DENSE_VALUES, size=(rows, fan), p=DENSE_P)
            if density < 1.0:
                w = w * (rng.uniform(size=(rows, fan)) < density)
        else:
            # support uniform over (c_in, tap); the first entry of row r is stratified over the input channels (channel
            # perm[r mod c_in], any tap), so that every channel is read by some row of a layer with as many rows as inputs
            w = np.zeros((rows, fan))
            taps = fan // shape[1]
            perm = rng.permutation(shape[1])
            for r in range(rows):
                idx = [int(perm[r % shape[1]]) * taps + int(rng.integers(taps))]
                while len(idx) < min(_ONE_PER_ROW.get(p, SPARSE_PER_ROW), fan):
                    j = int(rng.integers(fan))
                    if j not in idx:
                        idx.append(j)
                w[r, idx] = rng.choice((-1.0, 1.0), size=len(idx))
        b = _bias(rng, rows).astype(np.float64)
        if p in _HEAD_FIRST:
            w, b = w * HEAD_SCALE, b * HEAD_SCALE
        t[p + ".weight"] = w.reshape(shape).astype(np.float32)
        t[p + ".bias"] = b.astype(np.float32)
    if wide is not None:
        _widen(t, meta, names, wide, seed)
    return meta, t


def _side_rows(p, q, side):
    """Output rows of the attention head's convolutions that make up q_from ("from") or q_to ("to")."""
    if p == "policy_head.conv_bulk":
        return np.arange(q) if side == "from" else np.arange(q, 2 * q)
    return np.arange(0) if side == "from" else np.arange(3 * q)  # conv_under: all of q_to


def _widen(t, meta, names, wide, seed):
    """The wide family, from the narrow draw (a pass of its own with a generator of its own: the narrow network of the same
    seed is the starting point).  wide = (at, side).  at = "input": nothing here (the scalar planes are wide, exact_boards);
    at = i: layer i gets FRAGMENT_ENTRIES more entries per weight fragment — (16 output rows, tap, 32 input channels) — and all its
    weights and biases times WIDE; everything in front of layer i is narrow, everything behind it carries lo halves.
    side (attention heads; None elsewhere) names the operand of q_from . q_to that stays narrow: channels c with
    c % LANE == LANE - 1 read only such channels from the stem on (the stem's read the bool planes where the scalar planes are
    wide) and take no wide weight, the rows of that operand read only those channels, and its
    query channels are thinned out (NARROW_Q, NARROW_ON)."""
    at, side = wide
    rng = np.random.default_rng([seed, 15485863])
    ns, nb = meta["input_scalar_channels"], meta["input_bool_channels"]
    q = meta.get("policy_query_channels", 0)
    plain = {}  # layer -> the rows that may go wide
    for p in names:
        w = t[p + ".weight"]
        rows = np.arange(w.shape[0])
        if side is not None:
            if p.startswith("common.tower."):
                narrow = rows[rows % LANE == LANE - 1]
            elif p in _ONE_PER_ROW:
                narrow = _side_rows(p, q, side)
            else:
                narrow = rows[:0]
            stem = p == "common.tower.0"
            for r in narrow:  # move every entry of the row to a narrow input channel, same tap
                old, w[r] = w[r].copy(), 0.0
                for c in np.flatnonzero(old.reshape(old.shape[0], -1).any(axis=1)):
                    to = (ns + c % nb if at == "input" and c < ns else c) if stem else c - c % LANE + LANE - 1
                    w[r, to] = np.where(old[c] != 0, old[c], w[r, to])
            const = narrow[:0]
            if p in _ONE_PER_ROW and len(narrow):
                qi = (narrow if p == "policy_head.conv_bulk" else narrow // 3) % q
                const = narrow[qi % max(1, q // NARROW_Q) != 0]
                off = narrow[qi % max(1, q // NARROW_ON) != 0]
                w[const] = 0.0
                bias = t[p + ".bias"]
                bias[const] = np.where(bias[const] != 0, bias[const], HEAD_SCALE * rng.choice((-1.0, 1.0), size=len(const)))
                bias[off] = 0.0
            # a moved entry may have been the only one that read its channel: every input channel is read again, a wide one
            # (c % LANE != LANE - 1, or a scalar plane where those are wide) by a row that may be wide
            free = np.setdiff1d(rows, narrow)
            w3 = w.reshape(w.shape[0], w.shape[1], -1)
            for c in np.flatnonzero(~w3.any(axis=(0, 2))):
                lane_in = c >= ns if stem else c % LANE == LANE - 1
                pick = np.setdiff1d(rows, const) if lane_in or (stem and at != "input") else free
                if not len(pick):
                    continue  # (conv_under with q_to narrow: nothing of it may read a wide channel)
                w3[int(rng.choice(pick)), c, int(rng.integers(w3.shape[2]))] = (HEAD_SCALE if p in _HEAD_FIRST else 1.0) * rng.choice((-1.0, 1.0))
            rows = np.setdiff1d(rows, narrow)
        plain[p] = rows
    if at == "input":
        return
    p = names[at]
    w, rows = t[p + ".weight"], plain[p]
    w3 = w.reshape(w.shape[0], w.shape[1], -1)  # (a view: 2-D weights have one tap)
    unit = HEAD_SCALE if p in _HEAD_FIRST else 1.0
    for r0 in range(0, w.shape[0], 16):
        tile = rows[(rows >= r0) & (rows < r0 + 16)]
        if not len(tile):
            continue
        for tap in range(w3.shape[2]):
            for c0 in range(0, w.shape[1], 32):
                for _ in range(FRAGMENT_ENTRIES):
                    r, c = int(rng.choice(tile)), c0 + int(rng.integers(min(32, w.shape[1] - c0)))
                    if w3[r, c, tap] == 0:
                        w3[r, c, tap] = unit * rng.choice((-1.0, 1.0))
    w[rows] *= np.float32(WIDE)
    t[p + ".bias"][rows] *= np.float32(WIDE)  # (f32 in every kernel: the accumulator starts wide, so the output is wide wherever the bias is not zero)


def _bias(rng, n):
    b = rng.integers(-1, 2, size=n).astype(np.float32)
    if not b.any():
        b[rng.integers(n)] = 1.0
    return b


def draw_exact(game, depth, channels, head, dense_at, seed, density=1.0, boards=None, max_redraws=8, wide=None, **kw):
    """(meta, tensors, seed used, (scalars, policy, report) of `reference` on the boards).  Redraws the seed until the
    reference meets the conditions.  With the weights drawn, one pass of the reference over the boards raises the integer
    bias in front of every ReLU whose channel would be positive on less than LIVE_SHARE of the (board, square) positions
    (`revive`): a weight that reads a dead channel could be anything, and one that reads a channel alive on a few squares
    only shows where the ReLU behind it happens to be open.  wide = (at, side): a network of the wide family (`_widen`)."""
    bits, scalars = boards if boards is not None else exact_boards(game, 13, seed, wide=wide is not None and wide[0] == "input")
    for attempt in range(max_redraws):
        s = seed + 1000 * attempt
        meta, t = _draw(game, depth, channels, head, dense_at, s, density, kw, wide)
        out = reference(t, meta, encode(meta, bits, scalars), revive=True)
        if conditions_hold(out[2], wide is not None):
            return meta, t, s, out
    raise RuntimeError(f"no exact network in {max_redraws} draws: {game} {depth}x{channels} {head} dense_at={dense_at}")


def exact_model(game, depth, channels, head, dense_at, seed, **kw):
    """(blob, tensors).  The layer numbered `dense_at` (layer_names order; None: no such layer) has no zero weight, drawn from
    DENSE_VALUES — every weight position of it moves an integer output by at least 1 wherever its input is non-zero —,
    every other layer two +-1 entries per output row.  Keywords: draw_exact's (density, boards, max_redraws) and
    synth.random_model's."""
    meta, t, _, _ = draw_exact(game, depth, channels, head, dense_at, seed, **kw)
    return write_model(meta, t), t


def exact_boards(game, batch, seed, wide=False):
    """Bool planes as synth.random_boards; scalars small integers (Ataxx, and Go's komi plane: halves) in place of the raw counters.
    wide: every scalar s becomes (s + 1) * WIDE — no plane is zero, every one has a lo half."""
    bits, scalars = synth.random_boards(game, batch, seed=seed)
    rng = np.random.default_rng([seed, 104729])
    if game.startswith("ataxx"):
        scalars = rng.integers(0, 3, size=scalars.shape) / 2.0
    elif game.startswith("go"):
        scalars = scalars.copy()
        scalars[:, 4] = rng.integers(0, 3, size=batch) / 2.0  # komi plane (7.5 / 15 in random_boards)
    elif scalars.shape[1]:
        keep = scalars <= 2  # flags and repetition counts stay; the 0..99 / 0..59 counters become 0..2
        scalars = np.where(keep, scalars, rng.integers(0, 3, size=scalars.shape))
    if wide:
        scalars = (scalars + 1.0) * WIDE
    return bits, np.ascontiguousarray(scalars, dtype=np.float32)


def encode(meta, bits, scalars):
    """encode_input_full: scalar planes broadcast over the board, then the bool planes (LSB-first bits)."""
    h, w = meta["board_h"], meta["board_w"]
    ns, nb = meta["input_scalar_channels"], meta["input_bool_channels"]
    b = bits.shape[0]
    planes = np.unpackbits(bits, axis=1, bitorder="little")[:, :nb * h * w].reshape(b, nb, h, w)
    x = np.empty((b, ns + nb, h, w), np.float64)
    x[:, :ns] = scalars.astype(np.float64)[:, :, None, None]
    x[:, ns:] = planes
    return x


# ---- the float64 reference ----

def step_of(v):
    """Largest power of two dividing every value of v (1.0 for an all-zero tensor)."""
    v = np.asarray(v, np.float64).ravel()
    v = v[v != 0]
    if v.size == 0:
        return 1.0
    m, e = np.frexp(np.abs(v))
    mi = (m * 2.0 ** 53).astype(np.int64)
    tz = np.log2((mi & -mi).astype(np.float64)).astype(np.int64)
    return float(2.0 ** int((e - 53 + tz).min()))


def f16_neighbours(v):
    """The f16 values just below and just above v (both v itself where f16 holds it)."""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
    inf = np.float16(np.inf)
    return np.where(h > v, np.nextafter(h, -inf), h), np.where(h < v, np.nextafter(h, inf), h)


def split16(v):
    """(hi, lo) in float64 as the kernels form them: hi = f16(v), lo = f16(v - hi), to nearest."""
    v = np.asarray(v, np.float64)
    hi = v.astype(np.float16).astype(np.float64)
    return hi, (v - hi).astype(np.float16).astype(np.float64)


def split_exact(v):
    """(v == hi + lo with lo = f16(v - hi) and no non-zero |lo| below LO_MIN, for hi either f16 neighbour of v — no
    rounding mode of the conversion is assumed — and max |v| <= SPLIT_MAX; some lo is non-zero)."""
    v = np.asarray(v, np.float64)
    if np.abs(v).max(initial=0.0) > SPLIT_MAX:
        return False, True
    ok, any_lo = True, False
    for hi in f16_neighbours(v):
        lo = (v - hi.astype(np.float64)).astype(np.float16).astype(np.float64)
        ok = ok and bool(np.array_equal(hi.astype(np.float64) + lo, v)) and not bool(((lo != 0) & (np.abs(lo) < LO_MIN)).any())
        any_lo = any_lo or bool(lo.any())
    return ok, any_lo


class _Report:
    def __init__(self, measure=True, light=False):
        self.measure = measure
        self.light = light  # the rounding family: sums, f32 exactness and the rounding counts; nothing of the f16 / split16 conditions
        self.stored = {}  # name -> (max |v| / step, round-trips through f16)
        self.sums = {}    # name -> max sum |a b| / step
        # what the wide family adds (narrow networks hold all of it trivially, every lo being zero)
        self.split = {}   # name (a stored tensor, or "<layer>.weight") -> (split_exact, step >= LO_MIN or no lo at all)
        self.lolo = {}    # product -> (one operand has no lo half, hi*hi + hi*lo + lo*hi == the plain result)
        self.lo_in = {}   # layer -> (share of its input's entries with a lo half, every 32-channel chunk has one)
        self.lo_w = {}    # layer -> [tile, chunk, tap] bool: that weight fragment (16 rows, tap, 32 input channels) holds a lo half
        # what the rounding family adds (`rounding=` of `reference`)
        self.ties = {}    # rounding site (a stored tensor, or a layer: its weights) -> (ties rounded down, ties rounded up, non-ties) by bf16_rne
        self.f32 = {}     # stored tensor, and "<site>.before" for what a site rounds -> finite and exact in f32
        self.values = {}  # every tensor a site could round (a stored tensor, a layer's weights) -> what was carried on

    def count(self, name, v):
        """A rounding site's input by what round-to-nearest-even to bf16 does to it (magnitudes: down is towards zero)."""
        self.f32[name + ".before"] = f32_exact(v)
        lo, frac, _ = _bf16_parts(v)
        tie = frac == 0.5
        self.ties[name] = (int((tie & (lo % 2 == 0)).sum()), int((tie & (lo % 2 == 1)).sum()), int(((frac != 0) & ~tie).sum()))

    def store(self, name, v):
        if not self.measure:
            return
        self.f32[name] = f32_exact(v)
        if self.light:
            return
        ok = bool(np.array_equal(v.astype(np.float16).astype(np.float64), v))
        self.stored[name] = (float(np.abs(v).max() / step_of(v)), ok)
        ok, any_lo = split_exact(v)
        self.split[name] = (ok, not any_lo or step_of(v) >= LO_MIN)

    def acc(self, name, mag, step):
        self.sums[name] = float(mag.max() / step)

    def worst(self):
        return max(v for v, _ in self.stored.values()), max(self.sums.values())


def conditions_hold(report, wide=False):
    """Narrow family: stored and sums.  Wide family: split-stored, no lo.lo, sums."""
    sums = all(v <= SUM_MAX for v in report.sums.values())
    if wide:
        return sums and all(a and b for a, b in report.split.values()) and all(a and b for a, b in report.lolo.values())
    return sums and all(ok and v <= STORED_MAX for v, ok in report.stored.values())


def _chunks(a, n, axis):
    """a with `axis` cut into pieces of n (the last one padded with zeros) -> [..., pieces, n, ...]."""
    pad = -a.shape[axis] % n
    a = np.pad(a, [(0, pad if i == axis else 0) for i in range(a.ndim)])
    return a.reshape(a.shape[:axis] + (a.shape[axis] // n, n) + a.shape[axis + 1:])


def _edge(hh, ww):
    m = np.zeros((hh, ww), bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def _lin(x, w, spoil=None, mags=True):
    """w applied to x without the bias (3x3 same-padded: nine shifted einsums on a zero-padded image; 1x1; any odd k; 2-D
    w: linear), and the same on the magnitudes.  spoil = (dy, dx): what a wrong lo address of the input does — on that tap
    the board's edge squares read x without its lo halves.  mags=False: the magnitudes are not wanted (None)."""
    if w.ndim == 2:
        return x @ w.T, np.abs(x) @ np.abs(w).T if mags else None
    k = w.shape[2]
    pad = k // 2
    hh, ww = x.shape[2], x.shape[3]
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    y = np.zeros((x.shape[0], w.shape[0], hh, ww))
    mag = np.zeros_like(y) if mags else None
    for dy in range(k):
        for dx in range(k):
            win = xp[:, :, dy:dy + hh, dx:dx + ww]
            if spoil == (dy, dx):
                win = np.where(_edge(hh, ww), split16(win)[0], win)
            y += np.einsum("oc,bchw->bohw", w[:, :, dy, dx], win, optimize=True)
            if mags:
                mag += np.einsum("oc,bchw->bohw", np.abs(w[:, :, dy, dx]), np.abs(win), optimize=True)
    return y, mag


def _conv(rep, name, x, w, b, spoil=None):
    """Convolution or, for 2-D w, linear layer, with what the report measures of it.  spoil: {"tap": (dy, dx)} (`_lin`),
    {"fragment": (tile, (dy, dx), chunk)}: that weight fragment loses its lo halves, or {"chunk": k}: what a stale image chunk
    does in a kernel that stages its input 64 channels at a time — on the board's edge squares channels 64 k .. 64 k + 63 are read
    from chunk k - 1, for a k that is neither the first chunk nor the last (ValueError where the layer has no such chunk)."""
    w, b = w.astype(np.float64), b.astype(np.float64)
    spoil = spoil or {}
    if "chunk" in spoil:
        k, chunks = spoil["chunk"], x.shape[1] // 64
        if x.ndim != 4 or not 1 <= k <= chunks - 2:
            raise ValueError(f"{name}: {chunks} chunks of 64 input channels, none at {k} that is neither the first nor the last")
        x = x.copy()
        x[:, 64 * k:64 * k + 64] = np.where(_edge(x.shape[2], x.shape[3]), x[:, 64 * k - 64:64 * k], x[:, 64 * k:64 * k + 64])
    if "fragment" in spoil:
        tile, (dy, dx), chunk = spoil["fragment"]
        w = w.copy()
        part = w[16 * tile:16 * tile + 16, 32 * chunk:32 * chunk + 32, dy, dx]
        part[...] = split16(part)[0]
    y, mag = _lin(x, w, spoil.get("tap"), mags=rep.measure)
    shape = (1, -1) + (1,) * (y.ndim - 2)
    y = y + b.reshape(shape)
    if not rep.measure:
        return y
    rep.acc(name, mag + np.abs(b).reshape(shape), min(step_of(w) * step_of(x), step_of(b)))
    if rep.light:
        return y
    ok, any_lo = split_exact(w)
    rep.split[name + ".weight"] = (ok, not any_lo or step_of(w) >= LO_MIN)
    (xh, xl), (wh, wl) = split16(x), split16(w)
    three = _lin(xh, wh)[0] + (_lin(xl, wh)[0] if xl.any() else 0.0) + (_lin(xh, wl)[0] if wl.any() else 0.0) + b.reshape(shape)
    rep.lolo[name] = (not (xl.any() and wl.any()), bool(np.array_equal(three, y)))
    live = _chunks(xl != 0, 32, 1)
    rep.lo_in[name] = (float(np.mean(xl != 0)), bool(live.any(axis=tuple(i for i in range(live.ndim) if i != 1)).all()))
    frag = _chunks(_chunks(wl.reshape(wl.shape[0], wl.shape[1], -1) != 0, 16, 0), 32, 2)  # [tile, 16, chunk, 32, tap]
    rep.lo_w[name] = frag.any(axis=(1, 3))
    return y


def _bn(t, p, x, eps):
    y = (x - t[p + ".running_mean"].astype(np.float64)[None, :, None, None]) / np.sqrt(
        t[p + ".running_var"].astype(np.float64) + eps)[None, :, None, None]
    if p + ".weight" in t:
        y = y * t[p + ".weight"].astype(np.float64)[None, :, None, None] + t[p + ".bias"].astype(np.float64)[None, :, None, None]
    return y


def reference(t, meta, x, revive=False, spoil=None, exact=True, rounding=None):
    """(scalars [B, 5], policy [B, P], report) in float64; x [B, C_in, H, W].  report.acts holds the tower's and the scalar
    head's intermediates under the oracle's trace names.  revive (the generator's pass): t is changed in place — the bias
    in front of a ReLU is raised by whole units wherever the channel would be positive on too few positions.
    spoil = {"layer": name, "tap": (dy, dx)} or {"layer": name, "fragment": (tile, (dy, dx), chunk)}: one wrong lo address
    (`_conv`).  Three more, the faults of a kernel that stages 64 input channels at a time and writes 64 output channels per
    workgroup (tests/board_nets.py): {"layer": name, "chunk": k} (`_conv`); {"block": i, "quarter": q}: block i's residual on
    output channels 64 q .. 64 q + 63, q >= 2, is read from quarter q - 2; {"block": i, "stale": True}: block i's residual is
    block i - 1's input, what a rotation of activation buffers that never wraps would leave there.  Each raises ValueError on a
    network that has no such chunk, quarter or block.  exact=False: any network (random weights), nothing measured or asserted.
    rounding = (sites, fn): what a launch that rounds does (module docstring, "rounding").  At every `store` site named in
    sites the value is replaced by fn(value) and carried on, and so are the weights of every layer named there; fn is one
    function, or {site: function} with None as the key of the rest.  Two more sites exist for the mutants only: "tower.i.branch",
    block i's branch before the residual add, and "tower.<depth>", the last block's output.  The report counts per site
    what round-to-nearest-even would do (`ties`), keeps what each site carried on (`values`) and says whether every value in
    front of a rounding, and every stored one, is exact in f32 (`f32`); the f16 and split16 conditions are not measured."""
    rep = _Report(measure=exact, light=rounding is not None)
    acts = rep.acts = {}
    sites, fns = rounding if rounding is not None else (frozenset(), None)

    def rnd(name, v):
        fn = (fns.get(name, fns.get(None)) if isinstance(fns, dict) else fns) if name in sites else None
        if fn is None:
            if rounding is not None:
                rep.values[name] = v
            return v
        v = np.asarray(v, np.float64)
        if rep.measure:
            rep.count(name, v)
        rep.values[name] = fn(v)
        return rep.values[name]

    def relu(v, bias_key=None):
        if revive and bias_key is not None:
            unit = HEAD_SCALE if bias_key[:-len(".bias")] in _HEAD_FIRST else 1.0
            top = np.quantile(np.moveaxis(v, 1, 0).reshape(v.shape[1], -1), 1.0 - LIVE_SHARE, axis=1, method="higher")
            bump = np.where(top <= 0, np.ceil((unit - top) / unit) * unit, 0.0)
            if bump.any():
                bias = t[bias_key].astype(np.float64) + bump
                if not bias.any():  # (a bias of -1 raised by 1: keep the layer's bias non-zero somewhere)
                    bump = bump + unit * (bump > 0)
                    bias = t[bias_key].astype(np.float64) + bump
                t[bias_key] = bias.astype(np.float32)
                v = v + bump.reshape((1, -1) + (1,) * (v.ndim - 2))
        return np.maximum(v, 0.0)
    eps, depth = meta["bn_eps"], meta["tower_depth"]
    b = x.shape[0]

    def conv(p, v):
        return _conv(rep, p, v, rnd(p, t[p + ".weight"]), t[p + ".bias"], spoil if spoil and spoil.get("layer") == p else None)

    def residual(i, cur, before):
        """Block i's residual: its input — or what a wrong residual address reads (spoil["block"] == i)."""
        if not spoil or spoil.get("block") != i:
            return cur
        if "quarter" in spoil:
            q, quarters = spoil["quarter"], cur.shape[1] // 64
            if not 2 <= q < quarters:
                raise ValueError(f"block {i}: {quarters} output-channel quarters of 64, none at {q} with a quarter two below it")
            res = cur.copy()
            res[:, 64 * q:64 * q + 64] = cur[:, 64 * q - 128:64 * q - 64]
            return res
        if before is None:
            raise ValueError(f"block {i}: no block in front of it whose input a stale buffer could hold")
        return before

    if spoil and "block" in spoil and not 1 <= spoil["block"] <= depth:
        raise ValueError(f"block {spoil['block']}: the tower has {depth}")
    x = rnd("input", np.asarray(x, np.float64))
    rep.store("input", x)
    cur = rnd("tower.0", conv("common.tower.0", x))  # stem: no BN, no ReLU
    acts["tower.0"] = cur
    rep.store("tower.0", cur)
    before = None  # the previous block's input
    for i in range(1, depth + 1):
        p = f"common.tower.{i}.seq."
        mid = rnd(f"tower.{i}.mid", relu(_bn(t, p + "1", conv(p + "0", cur), eps), p + "1.bias"))
        acts[f"tower.{i}.mid"] = mid
        rep.store(f"tower.{i}.mid", mid)
        before, cur = cur, rnd(f"tower.{i}", residual(i, cur, before) + rnd(f"tower.{i}.branch", relu(_bn(t, p + "4", conv(p + "3", mid), eps), p + "4.bias")))  # the residual after the ReLU
        acts[f"tower.{i}"] = cur
        rep.store(f"tower.{i}", cur)
    common = rnd(f"tower.{depth + 1}", _bn(t, f"common.tower.{depth + 1}", cur, eps))
    acts[f"tower.{depth + 1}"] = common
    rep.store(f"tower.{depth + 1}", common)

    def hidden(name, v):
        v = rnd(name, v)
        rep.store(name, v)
        return v

    def scalar_branch(p, n0, n1, n2):  # conv1x1, ReLU, Flatten (channel-major), Linear, ReLU, Linear
        a = hidden(p + ".conv_relu", relu(conv(f"{p}.{n0}", common), f"{p}.{n0}.bias"))
        hid = hidden(p + ".fc0_relu", relu(conv(f"{p}.{n1}", a.reshape(b, -1)), f"{p}.{n1}.bias"))
        return a, hid, conv(f"{p}.{n2}", hid)

    a, hid, scalars = scalar_branch("scalar_head.seq", 0, 3, 5)
    acts["scalar_head.conv_relu"], acts["scalar_head.fc0_relu"] = a.reshape(b, -1), hid

    kind = meta["policy_kind"]
    if kind in ("ataxx_conv", "conv"):
        hid = hidden("policy_head.hidden", relu(conv("policy_head.seq.0", common), "policy_head.seq.0.bias"))
        policy = conv("policy_head.seq.2", hid).reshape(b, -1)
        if kind == "ataxx_conv":
            policy = np.concatenate([policy, np.zeros((b, 1))], axis=1)
        elif meta.get("policy_extra_moves", 0):
            e = hidden("policy_head.extra", conv("policy_head.seq_extra.0", common)).reshape(b, -1)
            policy = np.concatenate([policy, conv("policy_head.seq_extra.2", e)], axis=1)
    elif kind == "attention":
        q = meta["policy_query_channels"]
        bulk = conv("policy_head.conv_bulk", common)
        under = conv("policy_head.conv_under", common[:, :, 7:8, :])  # the last rank only
        q_from = hidden("policy_head.q_from", bulk[:, :q].reshape(b, q, 64))
        q_to = hidden("policy_head.q_to", np.concatenate([bulk[:, q:].reshape(b, q, 64), under.reshape(b, q, 24)], axis=2))
        logits = np.einsum("bqi,bqj->bij", q_from, q_to, optimize=True)
        if exact:
            rep.acc("policy_head.bmm", np.einsum("bqi,bqj->bij", np.abs(q_from), np.abs(q_to), optimize=True), step_of(q_from) * step_of(q_to))
            (fh, fl), (th, tl) = split16(q_from), split16(q_to)
            three = sum(np.einsum("bqi,bqj->bij", u, v, optimize=True) for u, v in ((fh, th), (fh, tl), (fl, th)))
            rep.lolo["policy_head.bmm"] = (not (fl.any() and tl.any()), bool(np.array_equal(three, logits)))
        policy = (logits / np.sqrt(float(q))).reshape(b, -1)[:, t["policy_head.FLAT_TO_ATT"]]
    elif kind == "dense":
        cur, idx = common, 0
        if meta.get("policy_dense_hidden_channels", 0):
            cur, idx = hidden("policy_head.hidden_conv", relu(conv("policy_head.seq.0", common), "policy_head.seq.0.bias")), 2
        cur, idx = cur.reshape(b, -1), idx + 1
        if meta.get("policy_dense_hidden_size", 0):
            cur, idx = hidden("policy_head.hidden_fc", relu(conv(f"policy_head.seq.{idx}", cur), f"policy_head.seq.{idx}.bias")), idx + 2
        policy = conv(f"policy_head.seq.{idx}", cur)
    elif kind == "arimaa":
        hid = hidden("policy_head.bulk_hidden", relu(conv("policy_head.bulk.0", common), "policy_head.bulk.0.bias"))
        bulk = conv("policy_head.bulk.2", hid).reshape(b, -1)
        _, _, sc = scalar_branch("policy_head.scalar", 0, 3, 5)
        policy = np.concatenate([sc, bulk], axis=1)
    else:
        raise ValueError(f"no exact reference for policy head '{kind}'")
    # the outputs are f32: they must be exact there
    for name, v in (("scalars", scalars), ("policy", policy)) if exact else ():
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), f"{name}: not exact in f32"
    return scalars, policy, rep


# ---- the committed networks: one per shape a kernel instance addresses on its own (tests/test_gpu_exact.py lists the engines) ----
# (game, depth, channels, head, synth.random_model keywords, {dense position: density < 1 where full density leaves the headroom})
# — every position of every network below holds the conditions at full density, so the last field is empty throughout.
# Attention heads away from 256 channels take 64 query channels: 1 / sqrt(64) is a power of two like 1 / sqrt(256), 1 / sqrt(128) is not.
_Q64 = dict(query_channels=64)
NETS = {
    "chess_2x256_att": ("chess", 2, 256, "attention", {}, {}),
    "chess_1x256_att": ("chess", 1, 256, "attention", {}, {}),
    "chesshist1_1x256_att": ("chess-hist-1", 1, 256, "attention", {}, {}),
    "chesshist3_1x256_att": ("chess-hist-3", 1, 256, "attention", {}, {}),
    "chess_1x128_att": ("chess", 1, 128, "attention", _Q64, {}),
    "chess_1x192_att": ("chess", 1, 192, "attention", _Q64, {}),
    "chess_1x512_att": ("chess", 1, 512, "attention", _Q64, {}),  # (full density holds at 512 channels too)
    "ataxx7_1x128": ("ataxx-7", 1, 128, "ataxx_conv", {}, {}),
    "ataxx5_1x128": ("ataxx-5", 1, 128, "ataxx_conv", {}, {}),
    "ataxx7_1x64": ("ataxx-7", 1, 64, "ataxx_conv", {}, {}),
    "ataxx7_1x48": ("ataxx-7", 1, 48, "ataxx_conv", {}, {}),
    "ataxx6_1x128_sh96": ("ataxx-6", 1, 128, "ataxx_conv", dict(scalar_hidden_size=96), {}),
    "go9_1x128": ("go-9", 1, 128, "conv", {}, {}),
    "go9_1x256": ("go-9", 1, 256, "conv", {}, {}),
    "go9_1x96": ("go-9", 1, 96, "conv", {}, {}),
    "go19_1x64": ("go-19", 1, 64, "conv", {}, {}),
    "go19_1x128": ("go-19", 1, 128, "conv", {}, {}),
    "go13_1x128": ("go-13", 1, 128, "conv", {}, {}),
    "chess_1x128_dense": ("chess", 1, 128, "dense", dict(dense_hidden_channels=8, dense_hidden_size=64), {}),
    "arimaa_1x96": ("arimaa-split", 1, 96, "arimaa", {}, {}),
    "ttt_1x32_dense": ("ttt", 1, 32, "dense", {}, {}),
}
SEED = 1
BOARDS = 13  # every engine evaluates slices of these: the conditions are measured on all of them


def positions(net):
    """None and every layer index of the network."""
    game, depth, channels, head, kw, _ = NETS[net]
    _, t = read_model(synth.random_model(game, depth, channels, head, seed=SEED, **kw))
    return [None] + list(range(len(layer_names(t))))


# The wide family: the networks a split16 engine runs (tests/test_gpu_exact.py), no dense layer.
WIDE_NETS = ("chess_2x256_att", "chess_1x128_att", "chess_1x192_att", "ataxx7_1x128", "ataxx5_1x128", "ataxx7_1x64",
             "go9_1x128", "go19_1x64", "go19_1x128")


def wide_positions(net):
    """(at, side) of every wide variant of a network: the scalar planes wide ("input"), then each layer's weights in turn.
    Attention heads: each variant twice, q_from or q_to the narrow operand; conv_under makes up q_to only, so it is wide
    with q_from narrow, and conv_bulk is wide on the other operand's rows: the two variants together cover its fragments."""
    game, depth, channels, head, kw, _ = NETS[net]
    _, t = read_model(synth.random_model(game, depth, channels, head, seed=SEED, **kw))
    names = layer_names(t)
    sides = ("from", "to") if head == "attention" else (None,)
    skip = ("policy_head.conv_under", "scalar_head.")  # (the scalar head's variants do not depend on the side: once)
    return [(at, side) for side in sides for at in ["input"] + list(range(len(names)))
            if not (side == "to" and at != "input" and names[at].startswith(skip))]


def wide_id(wide):
    return f"wide-{wide[0]}" + (f"-{wide[1]}" if wide[1] else "")


class Built:
    pass


_CACHE = {}
_COVER = {}  # (net, wide) -> (report.lo_in, report.lo_w): small, kept for every wide model built


def build(net, dense_at, wide=None):
    """One model per (network, dense position, wide variant), with its boards and float64 reference; cached (the last few
    only: the 512-channel blobs are tens of MB)."""
    key = (net, dense_at, wide)
    if key not in _CACHE:
        while len(_CACHE) >= 12:
            _CACHE.pop(next(iter(_CACHE)))
        game, depth, channels, head, kw, density_at = NETS[net]
        b = Built()
        b.bits, b.scalars_in = exact_boards(game, BOARDS, SEED, wide=wide is not None and wide[0] == "input")
        b.meta, b.tensors, b.seed, (s, p, b.report) = draw_exact(game, depth, channels, head, dense_at, SEED, boards=(b.bits, b.scalars_in),
                                                                 density=density_at.get(dense_at, 1.0), wide=wide, **kw)
        b.blob = write_model(b.meta, b.tensors)
        b.x = encode(b.meta, b.bits, b.scalars_in)
        b.ref_scalars, b.ref_policy = s.astype(np.float32), p.astype(np.float32)
        b.layers = layer_names(b.tensors)
        _CACHE[key] = b
        if wide is not None and dense_at is None:
            _COVER[net, wide] = (b.report.lo_in, b.report.lo_w)
    return _CACHE[key]


def coverage(net):
    """{wide variant: (lo_in, lo_w)} over every wide variant of the network."""
    for wide in wide_positions(net):
        if (net, wide) not in _COVER:
            build(net, None, wide)
    return {wide: _COVER[net, wide] for wide in wide_positions(net)}


# ---- the rounding family: a launch that rounds to bf16 (module docstring, "rounding") ----

def f32_exact(v):
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        return bool(np.isfinite(v).all() and np.array_equal(v.astype(np.float32).astype(np.float64), v))


def _bf16_parts(v):
    """|v| = (lo + frac) * 2^(e - 8): lo the integer that holds the 8 significant bits a bf16 value has (128 .. 255; 0 for
    v = 0), frac in [0, 1) what is beyond them.  Exact in float64 for a v that is exact in f32."""
    m, e = np.frexp(np.abs(np.asarray(v, np.float64)))  # m in [0.5, 1)
    lo = np.floor(m * 256.0)
    return lo, m * 256.0 - lo, e


def _bf16(v, up_if):
    v = np.asarray(v, np.float64)
    assert f32_exact(v) and np.abs(v).max(initial=0.0) < 2.0 ** 127 and (np.abs(v[v != 0]) > 2.0 ** -120).all(), "bf16: f32 values in the normal range"
    lo, frac, e = _bf16_parts(v)
    return np.copysign(np.ldexp(lo + up_if(lo, frac), e - 8), v)


def bf16_rne(v):
    """The nearest value with 8 significant bits, a tie to the one whose last bit is zero — from the definition."""
    return _bf16(v, lambda lo, frac: (frac > 0.5) | ((frac == 0.5) & (lo % 2 == 1)))


def bf16_trunc(v):
    """(mutant) the upper half of the f32: towards zero."""
    return _bf16(v, lambda lo, frac: np.zeros(lo.shape, bool))


def bf16_half_away(v):
    """(mutant) to nearest, a tie away from zero."""
    return _bf16(v, lambda lo, frac: frac >= 0.5)


def bf16_sites(meta, heads_inside):
    """(stored tensors the bf16 launch rounds, layers whose weights it holds in bf16), from kz_tower_pairs.hpp with BF = true:
    the staged input planes (split4<E>), the stem's epilogue into X, conv A's epilogue into Y (`tower.i.mid`), conv B's epilogue
    into X for every block but the last — ReLU and residual add in f32 in front of the one conversion —; the last layer's
    epilogue rounds only with the heads inside, and then behind the final BN (`tower.<depth + 1>`; the last block's own output
    exists in f32 registers only), and so does the policy head's hidden layer, one more pass of the weight stream into Y.  The
    weight stream — stem, blocks, and that pass — is packed to bf16 on the host (element_bits); the heads' tail reads the two
    images and f32 weights."""
    depth = meta["tower_depth"]
    sites = ["input", "tower.0"] + [f"tower.{i}.mid" for i in range(1, depth + 1)] + [f"tower.{i}" for i in range(1, depth)]
    weights = ["common.tower.0"] + [f"common.tower.{i}.seq.{j}" for i in range(1, depth + 1) for j in (0, 3)]
    if heads_inside:
        sites += [f"tower.{depth + 1}", "policy_head.hidden"]
        weights += ["policy_head.seq.0"]
    return sites, weights


# scalar planes and weights times one of these: two ties (to the even neighbour below, to the even neighbour above), two values
# that are no tie (just above the first tie, just below the upper neighbour), one that bf16 holds
ROUND_FACTORS = (1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -12, 1 + 2.0 ** -7 - 2.0 ** -12, 1 + 2.0 ** -7)
ROUND_THIN = {256: 8, 64: 4}  # attention heads: one query channel in this many is on (every sum <= SUM_MAX; more where a case needs it)


def round_boards(game, batch, seed):
    """exact_boards with every scalar s replaced by (s + 1) f, f drawn per entry from ROUND_FACTORS."""
    bits, scalars = exact_boards(game, batch, seed)
    f = np.random.default_rng([seed, 1299709]).choice(ROUND_FACTORS, size=scalars.shape)
    return bits, np.ascontiguousarray((scalars.astype(np.float64) + 1.0) * f, dtype=np.float32)


def _thin_queries(t, q, every):
    """Both operands of q_from . q_to are zero, bias included, on all but one query channel in `every`."""
    for p in _ONE_PER_ROW:
        rows = np.arange(t[p + ".weight"].shape[0])
        off = rows[((rows if p == "policy_head.conv_bulk" else rows // 3) % q) % every != 0]
        t[p + ".weight"][off] = 0.0
        t[p + ".bias"][off] = 0.0


def _read_every_channel(t, p, rng):
    """The narrow draw gives a layer with few output rows (the policy head's last one: 17 moves, or one) two entries per row,
    so most channels of the rounded hidden layer in front of it would be read by nothing: one +-1 entry more per such channel."""
    w = t[p + ".weight"]
    w3 = w.reshape(w.shape[0], w.shape[1], -1)  # (a view)
    for c in np.flatnonzero(~w3.any(axis=(0, 2))):
        w3[int(rng.integers(w.shape[0])), c, int(rng.integers(w3.shape[2]))] = rng.choice((-1.0, 1.0))


def round_conditions_hold(report):
    return all(v <= SUM_MAX for v in report.sums.values()) and all(report.f32.values())


def draw_rounding(game, depth, channels, head, variant, seed, heads_inside, max_redraws=4, **kw):
    """A network of the rounding family, from the narrow draw: a Built with the boards, the rounding reference (`ref_*`, `report`,
    `rounding`), the seed and the thinning used, and for the input variant the unrounded reference (`plain_*`) an exact-f32
    engine must return.  Variants:
      ("dense", at, gain)  layer `at` (layer_names order) dense, its weights times the odd gain: what it sums has more than 8 bits;
      ("input",)           the scalar planes need rounding (round_boards): every site at once, the stem's output included;
      ("weights", at)      layer `at` dense and half of its weights times a factor of ROUND_FACTORS: the host's packing rounds
                           (and so does everything behind that layer).
    Attention heads multiply two activations: one query channel in ROUND_THIN is on, fewer where the sums ask for it; the input
    variant, whose unrounded twin carries 13 more bits through the whole tower, keeps q_from narrow the way the wide family
    does (`_widen`, at = "input").  Accepted if `rounded` and `sums` hold (and for the unrounded twin `sums`, f32 exactness of
    every stored tensor and of the outputs); else thinned further, then redrawn."""
    kind = variant[0]
    att = head == "attention"
    bits, scalars = round_boards(game, BOARDS, seed) if kind == "input" else exact_boards(game, BOARDS, seed)
    for attempt in range(max_redraws):
        s = seed + 1000 * attempt
        q = thin = None
        while True:
            meta, t = _draw(game, depth, channels, head, None if kind == "input" else variant[1], s, 1.0, kw,
                            ("input", "from") if att and kind == "input" else None)
            names = layer_names(t)
            if att:
                q = meta["policy_query_channels"]
                thin = ROUND_THIN[q] if thin is None else 2 * thin
                if thin > q:
                    break
                _thin_queries(t, q, thin)
            if heads_inside:
                _read_every_channel(t, "policy_head.seq.2", np.random.default_rng([s, 49979687]))
            if kind == "dense":
                assert variant[2] % 2 == 1 and variant[2] <= 7
                t[names[variant[1]] + ".weight"] *= np.float32(variant[2])
            elif kind == "weights":
                assert heads_inside, "the attention head outside the launch multiplies two long operands in f32"
                rng = np.random.default_rng([s, 32452843, variant[1]])
                w = t[names[variant[1]] + ".weight"]
                f = rng.choice(ROUND_FACTORS, size=w.shape).astype(np.float32)
                w *= np.where(rng.uniform(size=w.shape) < 0.5, f, np.float32(1.0))
            sites, weights = bf16_sites(meta, heads_inside)
            rounding = (frozenset(sites + weights), bf16_rne)
            x = encode(meta, bits, scalars)
            try:
                out = reference(t, meta, x, revive=True, rounding=rounding)
                ok = round_conditions_hold(out[2])
                plain = reference(t, meta, x, rounding=(frozenset(), None)) if ok and kind == "input" else None
                ok = ok and (plain is None or round_conditions_hold(plain[2]))
            except AssertionError:  # (outputs not exact in f32, or a value in front of a rounding that is not)
                ok = False
            if ok:
                b = Built()
                b.bits, b.scalars_in, b.x, b.meta, b.tensors, b.seed, b.thin = bits, scalars, x, meta, t, s, thin
                b.variant, b.heads_inside, b.rounding, b.sites, b.weights = variant, heads_inside, rounding, sites, weights
                b.ref64, b.report = out[:2], out[2]
                b.ref_scalars, b.ref_policy = out[0].astype(np.float32), out[1].astype(np.float32)
                if plain is not None:
                    b.plain_report = plain[2]
                    b.plain_scalars, b.plain_policy = plain[0].astype(np.float32), plain[1].astype(np.float32)
                b.blob = write_model(meta, t)
                b.layers = names
                return b
            if not att:
                break
    raise RuntimeError(f"no rounding network in {max_redraws} draws: {game} {depth}x{channels} {head} {variant}")


# The smallest networks that take each branch of the bf16 template: (game, depth, channels, head, keywords, heads inside the launch)
ROUND_NETS = {
    "ataxx7_2x128": ("ataxx-7", 2, 128, "ataxx_conv", {}, True),        # heads inside, two-plane images
    "go9_3x128": ("go-9", 3, 128, "conv", {}, True),                    # heads inside, the pass move, depth 3: two block boundaries
    "chess_2x256_att": ("chess", 2, 256, "attention", {}, False),       # one-plane image, heads outside
    "chess_1x192_att": ("chess", 1, 192, "attention", _Q64, False),     # depth 1: the last-layer epilogue alone; the other channel mapping
}
# by depth: what the dense layer needs for values that are no tie behind it (gain 1: below 512, ties only).  A case that misses the
# coverage floors of tests/test_round_nets.py takes a larger odd gain in its variant, not a lower floor; none does.
ROUND_GAIN = {1: 5, 2: 3, 3: 3}


def round_variants(net):
    """Dense at every tower convolution whose output the launch stores in bf16 (heads outside: not the last one), and at the
    policy head's hidden layer with the heads inside; the input; the weights of every layer of the bf16 stream (heads inside)."""
    game, depth, channels, head, kw, inside = ROUND_NETS[net]
    _, t = read_model(synth.random_model(game, depth, channels, head, seed=SEED, **kw))
    names = layer_names(t)
    at = list(range(2 * depth + (1 if inside else 0))) + ([names.index("policy_head.seq.0")] if inside else [])
    out = [("dense", i, ROUND_GAIN[depth]) for i in at] + [("input",)]
    return out + ([("weights", i) for i in at] if inside else [])


def round_id(variant):
    return "-".join(str(v) for v in variant[:2])


_RCACHE = {}


def build_round(net, variant):
    """One network per (network, variant); cached (the last few only)."""
    if (net, variant) not in _RCACHE:
        while len(_RCACHE) >= 6:
            _RCACHE.pop(next(iter(_RCACHE)))
        game, depth, channels, head, kw, inside = ROUND_NETS[net]
        _RCACHE[net, variant] = draw_rounding(game, depth, channels, head, variant, SEED, inside, **kw)
    return _RCACHE[net, variant]


def round_mutants(b):
    """{name: rounding} of every reference that rounds otherwise than the launch is said to: another direction at every site
    (activations and weights), truncated weights alone, one site less — each in turn, the post-BN tower output with the heads
    inside among them —, the branch rounded in front of the residual add (two roundings), the last block's output rounded
    with the heads outside (the f32 rows that leave the launch)."""
    sites, weights = b.sites, b.weights
    both = frozenset(sites + weights)
    depth = b.meta["tower_depth"]
    m = {"truncate": (both, bf16_trunc), "half-away": (both, bf16_half_away),
         "truncated-weights": (both, {**{w: bf16_trunc for w in weights}, None: bf16_rne})}
    if not any(sum(b.report.ties[w]) for w in weights):
        del m["truncated-weights"]  # (every weight is a bf16 value: the same reference)
    for site in sites:
        if sum(b.report.ties[site]):  # (else nothing rounds there in this case: the same reference)
            m["without-" + site] = (both - {site}, bf16_rne)
    m["branch-rounded"] = (both | {f"tower.{i}.branch" for i in range(1, depth + 1)}, bf16_rne)
    if not b.heads_inside:
        m["last-block-rounded"] = (both | {f"tower.{depth}"}, bf16_rne)
    return m


def kept(report):
    """Every tensor the launch keeps, as the reference carried it on: the stream, the sites' values, the rounded weights."""
    return {k: v for k, v in report.values.items() if not k.endswith(".branch")}


def run_mutant(b, rounding):
    """(scalars, policy, some kept tensor differs from the rounding reference's) of a mutant reference, as f32."""
    s, p, rep = reference(b.tensors, b.meta, b.x, exact=False, rounding=rounding)
    base, mine = kept(b.report), kept(rep)
    applies = any(not np.array_equal(mine[k], base[k]) for k in mine if k in base)
    return s.astype(np.float32), p.astype(np.float32), applies


# ---- the scaled family: exact logits of any spread, for the decode (tests/decode_cases.py) ----

def logit_layers(meta, tensors):
    """[(layer, rows)] of every layer that writes a policy logit (rows None: all of them).  Conv and dense heads: the last
    layer (Go: the pass move's as well); the attention head: the q_from rows of conv_bulk — a logit is q_from . q_to / sqrt(q),
    linear in either operand."""
    kind = meta["policy_kind"]
    if kind in ("ataxx_conv", "conv"):
        return [("policy_head.seq.2", None)] + ([("policy_head.seq_extra.2", None)] if kind == "conv" and meta.get("policy_extra_moves", 0) else [])
    if kind == "attention":
        return [("policy_head.conv_bulk", _side_rows("policy_head.conv_bulk", meta["policy_query_channels"], "from"))]
    if kind == "dense":
        idx = (2 if meta.get("policy_dense_hidden_channels", 0) else 0) + 1 + (2 if meta.get("policy_dense_hidden_size", 0) else 0)
        return [(f"policy_head.seq.{idx}", None)]
    raise ValueError(f"no scaled family for policy head '{kind}'")


_SCACHE = {}


def build_scaled(net, k_policy, k_value, k_wdl):
    """`build(net, None)` with the layers that write the outputs times a power of two — exact, so the outputs are the base
    network's times that power, bit for bit, and a float64 softmax of them is a reference without logit error: every layer
    of `logit_layers` times 2^k_policy (weights and bias; a tuple: one exponent per layer, in that order), the rows of scalar_head.seq.5 times 2^k_value (row 0: value),
    2^k_wdl (rows 1-3) and 1 (row 4: moves left).  A Built with the base's boards, the reference rerun on the scaled tensors
    (`ref_scalars`, `ref_policy`, `report`), the base (`base`) and the exponents (`k`)."""
    key = (net, k_policy, k_value, k_wdl)
    if key not in _SCACHE:
        while len(_SCACHE) >= 6:
            _SCACHE.pop(next(iter(_SCACHE)))
        base = build(net, None)
        t = {k: v.copy() for k, v in base.tensors.items()}
        layers = logit_layers(base.meta, t)
        ks = k_policy if isinstance(k_policy, tuple) else (k_policy,) * len(layers)
        assert len(ks) == len(layers)
        for (p, rows), k in zip(layers, ks):
            rows = slice(None) if rows is None else rows
            t[p + ".weight"][rows] *= np.float32(2.0 ** k)
            t[p + ".bias"][rows] *= np.float32(2.0 ** k)
        f = np.array([2.0 ** k_value] + 3 * [2.0 ** k_wdl] + [1.0], np.float32)
        t["scalar_head.seq.5.weight"] *= f[:, None]
        t["scalar_head.seq.5.bias"] *= f
        b = Built()
        b.base, b.k, b.meta, b.tensors, b.seed = base, (k_policy, k_value, k_wdl), base.meta, t, base.seed
        b.bits, b.scalars_in, b.x, b.layers = base.bits, base.scalars_in, base.x, base.layers
        s, p, b.report = reference(t, b.meta, b.x)
        b.ref_scalars, b.ref_policy = s.astype(np.float32), p.astype(np.float32)
        b.blob = write_model(b.meta, t)
        _SCACHE[key] = b
    return _SCACHE[key]


def decode_ref(scalars, logits, move_lists):
    """decode_output (rust/kz-core/src/network/common.rs:16-100) in float64, from the definition: values [B, 5] =
    tanh(s0), softmax(s1..s3), s4 and per board the softmax over logits[moves] in the order given, the maximum subtracted,
    the sums by math.fsum (exactly rounded).  An empty list gives an empty array."""
    import math
    scalars, logits = np.asarray(scalars, np.float64), np.asarray(logits, np.float64)

    def softmax(v):
        e = np.exp(v - v.max())
        return e / math.fsum(e.tolist())
    values = np.empty((len(scalars), 5))
    values[:, 0] = np.tanh(scalars[:, 0])
    for b in range(len(scalars)):
        values[b, 1:4] = softmax(scalars[b, 1:4])
    values[:, 4] = scalars[:, 4]
    return values, [softmax(logits[b][np.asarray(m, np.int64)]) if len(m) else np.zeros(0) for b, m in enumerate(move_lists)]
