"""The decode (kz_decode_dev.hpp: tanh, the wdl softmax, gather and softmax over the listed moves) held to a float64
softmax of logits that are known exactly: the scaled family of tests/exact_nets.py (`build_scaled`), whose raw outputs
every path returns to the bit, with the layers that write them times a power of two — the spread of the logits is chosen
here, past the 88 at which a missed maximum overflows expf.  Shared by tests/test_decode_nets.py (no GPU: the family, the
shares of the error classes, the oracle's restatement inside the bounds, mutant decodes outside them) and
tests/test_gpu_decode_exact.py (every instantiation of decode_board_wave).

The bounds, against `exact_nets.decode_ref`, with u = 2^-24, n the length of a list and m = ceil(n / 64):
  probabilities  reference >= 2^-100 (the relative class): |out - ref| <= (m + 18) u ref — two exponentials of 3 ulp each enter
                 a quotient (4 * 3 u), a lane adds m positive terms and the wave six more ((m + 5) u), one division (u);
                 reference below 2^-100 (the underflow class): 0 <= out <= 2^-99;
                 a board's probabilities sum to 1 within n (m + 18) u;  the wdl triple: the same with m = 1;
  tanh           within 5 ulp (np.spacing) of the reference rounded to f32 — and exactly +-1 where the reference rounds to +-1;
  moves left     the bits of s4.
They are derived, not measured: no case may widen them.
"""
import math

import numpy as np

from kzero_amd import capi
from tests import exact_nets as E

U = 2.0 ** -24
REL_MIN, UNDER_MAX = 2.0 ** -100, 2.0 ** -99
F16, F32, SPLIT = capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F32_SPLIT16
GENERIC = {"KZ_FORCE_GENERIC": "1", "KZ_NO_BOARD_CONV": "1"}

# net -> (k_policy, k_wdl) of the wide variant, chosen so that the reference meets the conditions of tests/test_decode_nets.py
# (per board: spread > 104, indices at least 100 below the maximum; wdl spreads >= 88); k_value 5: every network has boards with
# |s0| > 9.02, where tanh rounds to +-1 in f32 (k_value 3 leaves Go 19x19 at |s0| <= 8 and tanh(8) = 1 - 3.8 ulp), beside smaller ones.
# The moderate variant: k_policy three less (every spread under 55: with the longest list's ln n <= 9.1 every probability
# stays above 2^-100 = e^-69.3), k_wdl 3, k_value -8 (s0 of a few thousandths: tanh's ulp bound where an absolute one is void).
K_WIDE = {
    "chess_2x256_att": (6, 5),     # spread 206 to 302
    "chess_1x128_att": (8, 6),     # 226 to 354; the largest wdl logit up to 160 above the second (k_wdl 5: 80, no overflow)
    "chess_1x128_dense": (5, 6),   # 320 to 360
    "ataxx7_1x128": (5, 5),        # 184 to 240
    "ataxx5_1x128": (5, 7),        # 144 to 180; wdl 96 to 320 (k_wdl 5: 24 to 80)
    # Go 9x9: the pass move leads every square by 2.25 to 3.25 and the squares span 1.4, so no common exponent puts entries both
    # within 69 and 100 below the maximum: the square layer (seq.2) and the pass layer (seq_extra.2) take one each — the
    # best squares are 64.2 below the pass move, the others down to 152; wdl 160 to 384
    "go9_1x128": ((6, -3), 7),
    "go19_1x64": (7, 5),           # 288 to 416, both the square and the pass layer
}
VARIANTS = ("wide", "moderate")
FAR, NEAR = 100.0, 64.0            # wide lists: the other entries at least FAR below the maximum; near lists: within NEAR of it


def exponents(net, variant):
    kp, kw = K_WIDE[net]
    if variant == "wide":
        return (kp, 5, kw)
    return (tuple(k - 3 for k in kp) if isinstance(kp, tuple) else kp - 3, -8, 3)


def scaled(net, variant):
    return E.build_scaled(net, *exponents(net, variant))


# `cap`: floats of LDS staging a wave has for one board's list (a longer list re-reads its tail), per instance, from the code:
STANDALONE = (1024, "kz_kernels.hip:792 DECODE_STAGE")
CHESS_F16 = (8448, "kz_tower.hip:699 64 * RS / 4, RS = 528 (:47)")
CHESS_SPLIT = (8448, "kz_tower_pairs.hpp:839 L::IMG / 4, Geo<256, 4, true>: IMG = 64 * 528 (:78-79)")


def tail_f16(nt):
    return (nt * 144, f"kz_conv_heads.hpp:201 stage_bytes / 16, kz_tower_pairs.hpp:614 L::IMG = {nt} * 16 * 144 (Geo<128, {nt}, false>, :78-79)")


def tail_f32(nt, where):
    return (nt * 528, f"kz_conv_heads.hpp:201 stage_bytes / 16, :267 rows_img * RS = {nt} * 16 * 528 ({where})")


# (id, network, dtype, max_batch, switches, tower path, boards per workgroup or None, boards of the ragged launch, (cap, where it is read), what decodes)
CASES = [
    ("chess256-f16-nb2", "chess_2x256_att", F16, 64, {}, "tower_resident_f16+heads", 2, 5, CHESS_F16, "kz_tower.hip, wave b decodes board b"),
    ("chess256-f16-nb1", "chess_2x256_att", F16, 64, {"KZ_TOWER_NB": "1"}, "tower_resident_f16+heads", 1, 3, CHESS_F16, "kz_tower.hip, one board"),
    ("chess256-split16", "chess_2x256_att", SPLIT, 64, {}, "tower_resident_split16+heads", 1, 5, CHESS_SPLIT, "kz_tower_pairs.hpp chess instance, wave 0"),
    ("chess256-f32", "chess_2x256_att", F32, 64, {}, "tower_resident_f32", 1, 9, STANDALONE, "kz_decode_output"),
    ("chess128-f16g", "chess_1x128_att", F16, 64, {}, "tower_resident_f16g", 1, 5, STANDALONE, "kz_decode_output"),
    ("chess128-dense-f16", "chess_1x128_dense", F16, 64, GENERIC, "conv_igemm_f16", None, 9, STANDALONE, "kz_decode_output, four boards per workgroup"),
    ("ataxx7x128-f16g-2", "ataxx7_1x128", F16, 64, {}, "tower_resident_f16g+heads", 2, 5, tail_f16(7), "conv_heads_tail"),
    ("ataxx7x128-f16g-4", "ataxx7_1x128", F16, 512, {}, "tower_resident_f16g+heads", 4, 509, tail_f16(13), "conv_heads_tail, one board per wave"),
    ("ataxx7x128-split16", "ataxx7_1x128", SPLIT, 64, {}, "tower_resident_split16+heads", 2, 9,
     tail_f32(7, "kz_tower_pairs.hpp:654 conv_heads_f32<128, 7>"), "conv_heads_tail"),
    ("ataxx7x128-f32", "ataxx7_1x128", F32, 64, {}, "tower_resident_f32+heads", 2, 9,
     tail_f32(7, "kz_tower_f32.hip:427, rows_img = ROWS, tiles_for :435"), "conv_heads_tail"),
    ("ataxx5x128-f16g", "ataxx5_1x128", F16, 64, {}, "tower_resident_f16g+heads", 4, 9, tail_f16(7), "conv_heads_tail, one board per wave"),
    ("go9x128-f16g-1", "go9_1x128", F16, 64, {}, "tower_resident_f16g+heads", 1, 3, tail_f16(6), "conv_heads_tail"),
    ("go9x128-f16g-2", "go9_1x128", F16, 256, {}, "tower_resident_f16g+heads", 2, 255, tail_f16(11), "conv_heads_tail"),
    ("go9x128-f16g-3", "go9_1x128", F16, 2048, {}, "tower_resident_f16g+heads", 3, 1534, tail_f16(16), "conv_heads_tail"),
    ("go9x128-f32", "go9_1x128", F32, 64, {}, "tower_resident_f32+heads", 1, 9,
     tail_f32(6, "kz_tower_f32.hip:427, rows_img = ROWS, tiles_for :435"), "conv_heads_tail"),
    ("go19x64-board-f16", "go19_1x64", F16, 256, {}, "board_conv_f16", None, 9, STANDALONE, "kz_decode_output"),
]
# every (network, cap) the GPU cases use: what tests/test_decode_nets.py holds without a GPU
NET_CAPS = sorted({(c[1], c[8][0]) for c in CASES})
LARGEST_CAP = max(c[8][0] for c in CASES)


# ---- move lists from the reference logits ----

def lengths(policy_len, cap):
    return sorted({1, 2, 63, 64, 65, 129, policy_len, cap - 1, cap, cap + 1, cap + 130})


def positions(n, cap):
    """Where the maximum sits: first entry, the first wrap's last lane, the second wrap's first, the last entry; a list longer
    than the staging also the last staged entry and one that only the re-read tail holds (behind the tail's first wrap where there is one)."""
    at = {0, 63, 64, n - 1}
    if n > cap:
        at |= {cap - 1, min(cap + 65, n - 1)}
    return sorted(j for j in at if 0 <= j < n)


class MoveList:
    def __init__(self, label, moves, at=None, same=None):
        self.label, self.moves, self.at, self.same = label, np.ascontiguousarray(moves, dtype=np.int32), at, same


def pools(logits, wide):
    """(index of the maximum, far pool, near pool): the indices FAR or more below the maximum (moderate: every index below it)
    and those within NEAR of it (at least four: else the four largest below it)."""
    top = int(np.argmax(logits))
    d = logits - logits[top]
    near = np.flatnonzero((d < 0) & (d >= -NEAR))
    if len(near) < 4:  # (a board whose maximum stands alone: its runners-up, whatever class they fall into)
        near = np.argsort(d, kind="stable")[-5:-1]
        near = near[d[near] < 0]
    return top, np.flatnonzero(d <= -FAR if wide else d < 0), near


def board_lists(logits, cap, wide, seed):
    """The lists of one board, from its reference logits (float64).  For every length and position of the maximum a far list:
    one entry is the maximum, every other one at least 100 below it (wide variant) — a maximum the decode misses overflows.
    Per length one near list (entries within 64 of the maximum: the relative class at every |l - max|), one list with the same
    index on both sides of the staging's end, one plain list (a random prefix of a permutation, as the other decode tests use).
    Indices repeat where a list is longer than its pool."""
    policy_len = len(logits)
    rng = np.random.default_rng([seed, 6700417])
    top, far, near = pools(logits, wide)
    assert len(far) and len(near), "no index far below / near the maximum: the network needs another k_policy"

    def fill(pool, n, at):
        rest = np.resize(rng.permutation(pool), n - 1)
        return np.concatenate([rest[:at], [top], rest[at:]])
    out = []
    for n in lengths(policy_len, cap):
        out += [MoveList(f"far-{n}-{at}", fill(far, n, at), at) for at in positions(n, cap)]
        out.append(MoveList(f"near-{n}", fill(near, n, n // 2), n // 2))
    n = cap + 130
    moves = fill(near, n, 0)
    moves[cap - 3] = moves[cap + 3] = near[len(near) // 2]
    out.append(MoveList("both-sides", moves, 0, same=(cap - 3, cap + 3)))
    out.append(MoveList("plain", rng.permutation(policy_len)[:int(rng.integers(1, policy_len + 1))]))
    return out


def schedule(batch, n_lists):
    """Which list every slot of a batch takes, round by round, until every (distinct board, list) has been decoded: slot i holds
    board (3 + i) mod 13 (tests/test_gpu_exact.py), and one slot per round is a finished board with no moves.
    -> (boards [batch], [per round: list number per slot, -1 for the empty one])."""
    boards = (3 + np.arange(batch)) % E.BOARDS
    todo = {(int(d), l) for d in set(boards.tolist()) for l in range(n_lists)}
    rounds = []
    while todo:
        r = len(rounds)
        pick = (np.arange(batch) + np.arange(batch) // E.BOARDS + r) % n_lists
        # the finished board: a slot whose list has been decoded already where there is one (else that list comes round again)
        done = [i for i in range(batch) if (int(boards[i]), int(pick[i])) not in todo]
        pick[done[(7 * r + 1) % len(done)] if done else (7 * r + 1) % batch] = -1
        todo -= {(int(d), int(l)) for d, l in zip(boards, pick)}
        rounds.append(pick)
        assert r < 4 * n_lists, "the schedule does not cover the lists"
    return boards, rounds


# ---- the bounds ----

class Worst:
    """The largest observed errors of a case, in units of u * ref and in tanh ulps."""
    def __init__(self):
        self.prob = self.share = self.wdl = self.tanh = self.under = 0.0

    def __str__(self):
        return (f"probs {self.prob:.2f} u ref ({self.share:.0%} of a list's bound at the most), wdl {self.wdl:.2f} u ref, "
                f"tanh {self.tanh:.2f} ulp, largest underflow-class output {self.under:.3g}")


def softmax_errors(out, ref, m):
    """Why `out` (f32) leaves the bounds of a softmax of n = len(ref) entries whose lanes add m terms ([]: it does not), and the
    largest relative error in units of u."""
    out64 = np.asarray(out, np.float64)
    n = len(ref)
    if not np.isfinite(out64).all():
        return [f"{int((~np.isfinite(out64)).sum())} of {n} not finite"], math.inf, 0.0
    rel = ref >= REL_MIN
    err = np.abs(out64[rel] - ref[rel]) / (U * ref[rel])
    why = []
    if (err > m + 18).any():
        i = int(np.flatnonzero(rel)[np.argmax(err)])
        why.append(f"entry {i}: {out64[i]!r} for {ref[i]!r}, {err.max():.1f} u ref > {m + 18}")
    under = out64[~rel]
    if ((under < 0) | (under > UNDER_MAX)).any():
        why.append(f"underflow class: outputs in [{under.min():g}, {under.max():g}]")
    if abs(math.fsum(out64.tolist()) - 1.0) > n * (m + 18) * U:
        why.append(f"sum {math.fsum(out64.tolist())!r}")
    return why, float(err.max(initial=0.0)), float(under.max(initial=0.0))


def probs_errors(out, ref, worst=None):
    m = -(-len(ref) // 64)
    why, err, under = softmax_errors(out, ref, m)
    if worst is not None:
        worst.prob, worst.share, worst.under = max(worst.prob, err), max(worst.share, err / (m + 18)), max(worst.under, under)
    return why


def values_errors(values, ref_values, s4, worst=None):
    """values [B, 5] (f32) against decode_ref's (float64) and the raw moves-left scalar (f32)."""
    why = []
    for b in range(len(values)):
        w, err, under = softmax_errors(values[b, 1:4], ref_values[b, 1:4], 1)
        why += [f"board {b} wdl: {x}" for x in w]
        t32 = np.float32(ref_values[b, 0])
        ulps = abs(float(values[b, 0]) - ref_values[b, 0]) / float(np.spacing(np.abs(t32))) if np.isfinite(values[b, 0]) else math.inf
        if abs(t32) == 1.0 and values[b, 0] != t32:
            why.append(f"board {b} tanh: {values[b, 0]!r}, not exactly {t32!r}")
        elif ulps > 5:
            why.append(f"board {b} tanh: {values[b, 0]!r} for {ref_values[b, 0]!r}, {ulps:.1f} ulp")
        if worst is not None:
            worst.wdl, worst.tanh, worst.under = max(worst.wdl, err), max(worst.tanh, ulps), max(worst.under, under)
    if not np.array_equal(np.asarray(values[:, 4], np.float32).view(np.uint32), np.asarray(s4, np.float32).view(np.uint32)):
        why.append("moves left: not the bits of s4")
    return why


# ---- the decode restated in f32, with a fault: what the bounds must catch ----

LOG2E = np.float32(1.4426950408889634)
FAULTS = ("max-first-64", "max-first-cap", "exp2")
WDL_FAULTS = ("wdl-max-without-s1", "wdl-max-without-s2", "wdl-max-without-s3")  # which two of the three: a case sees the one that drops its largest


def decode_f32(scalars, logits, move_lists, cap, fault=None):
    """kz_decode_dev.hpp's arithmetic in numpy float32 (differences, exponentials, quotients; the sum exactly rounded), and with
    `fault` one of FAULTS: the maximum over the first 64 entries only (one wrap of the wave), over the staged entries only,
    the exponential as exp2(x * log2 e) with the product rounded to f32; or one of WDL_FAULTS: the wdl maximum over two of the three."""
    scalars, logits = np.asarray(scalars, np.float32), np.asarray(logits, np.float32)

    def softmax(v, mx):
        with np.errstate(over="ignore", invalid="ignore"):
            d = v - mx
            e = np.exp2(d * LOG2E) if fault == "exp2" else np.exp(d)
            assert e.dtype == np.float32
            return e / np.float32(math.fsum(e.astype(np.float64).tolist()) if np.isfinite(e).all() else np.inf)
    values = np.empty((len(scalars), 5), np.float32)
    values[:, 0] = np.tanh(scalars[:, 0].astype(np.float64)).astype(np.float32)
    for b in range(len(scalars)):
        t = scalars[b, 1:4]
        values[b, 1:4] = softmax(t, np.delete(t, WDL_FAULTS.index(fault)).max() if fault in WDL_FAULTS else t.max())
    values[:, 4] = scalars[:, 4]
    probs = []
    for b, m in enumerate(move_lists):
        v = logits[b][np.asarray(m, np.int64)]
        seen = v[:64] if fault == "max-first-64" else v[:cap] if fault == "max-first-cap" else v
        probs.append(softmax(v, seen.max()) if len(v) else np.zeros(0, np.float32))
    return values, probs


# ---- one network, one staging size: the lists and their float64 decode, computed once per board and kept ----

class Reference:
    def __init__(self, net, cap, variant):
        self.net, self.cap, self.variant, self.wide = net, cap, variant, variant == "wide"
        self.b = scaled(net, variant)
        self.logits = self.b.ref_policy.astype(np.float64)
        self.values = E.decode_ref(self.b.ref_scalars, self.b.ref_policy, [[]] * E.BOARDS)[0]
        self._lists, self._probs = {}, {}

    def lists(self, board):
        if board not in self._lists:
            self._lists[board] = board_lists(self.logits[board], self.cap, self.wide, seed=board)
        return self._lists[board]

    def probs(self, board, l):
        """decode_ref of list l of the board (a view: nobody writes to it)."""
        if (board, l) not in self._probs:
            one = np.zeros((1, 5), np.float32)
            p = E.decode_ref(one, self.logits[board:board + 1], [self.lists(board)[l].moves])[1][0]
            p.setflags(write=False)
            self._probs[board, l] = p
        return self._probs[board, l]


_REFS = {}


def reference(net, cap, variant):
    if (net, cap, variant) not in _REFS:
        while len(_REFS) >= 2:
            _REFS.pop(next(iter(_REFS)))
        _REFS[net, cap, variant] = Reference(net, cap, variant)
    return _REFS[net, cap, variant]
