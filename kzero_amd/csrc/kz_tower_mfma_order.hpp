// kz_tower_mfma_order.hpp — the order in which one k-step of the f16 tower issues its MFMAs (host-includable: the table
// test tests/cpp/test_tower_mfma_order.cpp and the micro-benchmark tools/micro/mfma_order.hip read the same function the
// kernel does).
//
// A k-step multiplies NT = 4 weight fragments (the MFMA's A operand, af[nt]) with the line fragments of the tiles
// [lo, hi) of its tap row (the B operand, register bf[mt + dy]) into acc[nt][mt].  Every accumulator receives exactly one
// MFMA per k-step, so the order inside a k-step changes no sum; it changes how many operand registers differ between
// one MFMA and the next.  The walk is a boustrophedon: nt outermost, mt ascending under one nt and descending under the
// next, so that consecutive MFMAs of a k-step differ in exactly one of (nt, B register).
//
// The seams between the k-steps of a super-step (the three tap rows dy = -1, 0, +1 read the same eight B registers):
// NT is even, so a k-step ends on the tile it started on.  A k-step starts at the end of its range whose B register
// is the one the previous k-step ended on, if one of its two ends has it, and at lo otherwise.  This is a condition of
// the table, not a measurement.  For the line tiles (1..7 / 0..7 / 0..6) it gives: dy = -1 walks from tile 1 (register
// 0) and ends there; dy = 0 starts on tile 0 (register 0: carried); dy = +1 cannot carry it (its range reads
// registers 1..7) and starts on tile 0 (register 1).  The first k-step of a super-step reads the other register buffer
// and starts at lo.
// Distance between two MFMAs into the same accumulator: a tile's positions in two consecutive k-steps are at least
// (NT - 1) * (hi - lo) apart, because both k-steps start at the same end of their ranges or a whole nt row lies between.
#pragma once

namespace kz_mfma_order {

constexpr int NT = 4;  // output-channel tiles of a wave
static_assert(NT % 2 == 0, "a k-step ends on the tile it started on");

// the tap rows of a super-step: row i covers tiles [lo[i], hi[i]) and reads B register mt + dy[i]
struct Rows {
    int rows;
    int lo[3], hi[3], dy[3];
};
// line tiles (one tile per board line, MT tiles): the tile that dy puts outside the board is left out
constexpr Rows line_rows(int mt) { return Rows{3, {1, 0, 0}, {mt, mt, mt - 1}, {-1, 0, 1}}; }
// one tap row over all tiles (the 1x1 passes)
constexpr Rows one_row(int mt) { return Rows{1, {0, 0, 0}, {mt, 0, 0}, {0, 0, 0}}; }

struct Pos {
    int nt, mt;
};

constexpr int count(const Rows &r, int i) { return NT * (r.hi[i] - r.lo[i]); }

// position j of a boustrophedon over NT x [lo, hi) whose first nt row descends (desc) or ascends
constexpr Pos boustrophedon(int lo, int hi, bool desc, int j) {
    const int n = hi - lo, nt = j / n, k = j % n;
    return ((nt & 1) != 0) != desc ? Pos{nt, hi - 1 - k} : Pos{nt, lo + k};
}

// does k-step i start at the high end of its range (see the seam rule above)
constexpr bool starts_high(const Rows &r, int i) {
    if (i == 0) return false;
    const int prev = (starts_high(r, i - 1) ? r.hi[i - 1] - 1 : r.lo[i - 1]) + r.dy[i - 1];  // B register it ended on
    return r.lo[i] + r.dy[i] != prev && r.hi[i] - 1 + r.dy[i] == prev;
}

// (nt, mt) of the j-th MFMA of k-step i of a super-step, j in [0, count(r, i))
constexpr Pos at(const Rows &r, int i, int j) { return boustrophedon(r.lo[i], r.hi[i], starts_high(r, i), j); }

}  // namespace kz_mfma_order
