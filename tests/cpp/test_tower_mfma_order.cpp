// The MFMA order of a k-step of the chess f16 tower (kzero_amd/csrc/kz_tower_mfma_order.hpp), as a table: for the line
// tiles' tap rows (tiles 1..7 / 0..7 / 0..6 at dy = -1 / 0 / +1) and for one row over tiles 0..7,
//  * every (nt, mt in range) appears exactly once per k-step: every accumulator receives its one MFMA, no other does;
//  * consecutive MFMAs of a k-step differ in exactly one of (nt, B register mt + dy);
//  * at a dy seam the B register is unchanged wherever the next k-step's range has that register;
//  * no accumulator recurs within four positions, seams and the seam to the next super-step included.
// Host build of the header the kernel includes.
#include <cstdio>
#include <vector>

#include "../../kzero_amd/csrc/kz_tower_mfma_order.hpp"

namespace mo = kz_mfma_order;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// usable where the kernel uses it: in constant expressions
static_assert(mo::at(mo::line_rows(8), 0, 0).nt == 0 && mo::at(mo::line_rows(8), 0, 0).mt == 1, "dy = -1 starts on tile 1");
static_assert(mo::at(mo::line_rows(8), 1, 0).mt == 0 && mo::at(mo::line_rows(8), 2, 0).mt == 0, "dy = 0 and dy = +1 start on tile 0");
static_assert(mo::count(mo::line_rows(8), 0) == 28 && mo::count(mo::line_rows(8), 1) == 32 && mo::count(mo::line_rows(8), 2) == 28, "88 MFMAs");

struct Step {
    int i, nt, mt, breg;
};

static void check(const char *name, const mo::Rows &r, int mt_tiles) {
    std::vector<Step> super;  // one super-step, flattened
    int b_changes = 0, a_changes = 0, both = 0, ascending_b_changes = 0;
    for (int i = 0; i < r.rows; i++) {
        const int lo = r.lo[i], hi = r.hi[i], n = mo::count(r, i);
        EXPECT(n == mo::NT * (hi - lo), "%s k-step %d: count %d", name, i, n);
        std::vector<int> seen(mo::NT * mt_tiles, 0);
        for (int j = 0; j < n; j++) {
            const mo::Pos p = mo::at(r, i, j);
            EXPECT(p.nt >= 0 && p.nt < mo::NT && p.mt >= lo && p.mt < hi, "%s k-step %d position %d: (%d, %d) outside [%d, %d)", name, i, j, p.nt, p.mt, lo, hi);
            if (p.nt >= 0 && p.nt < mo::NT && p.mt >= 0 && p.mt < mt_tiles) seen[p.nt * mt_tiles + p.mt]++;
            const int breg = p.mt + r.dy[i];
            EXPECT(breg >= 0 && breg < mt_tiles, "%s k-step %d position %d: B register %d", name, i, j, breg);
            if (j > 0) {
                const Step &q = super.back();
                const bool da = q.nt != p.nt, db = q.breg != breg;
                EXPECT(da != db, "%s k-step %d positions %d, %d: (nt %d, B %d) -> (nt %d, B %d) changes %s", name, i, j - 1, j, q.nt, q.breg, p.nt, breg, da ? "both" : "neither");
                a_changes += da, b_changes += db, both += da && db;
            } else if (i > 0) {
                const Step &q = super.back();  // the seam
                const bool has = q.breg >= r.lo[i] + r.dy[i] && q.breg < r.hi[i] + r.dy[i];
                EXPECT(!has || breg == q.breg, "%s seam %d -> %d: B register %d -> %d, and the range has %d", name, i - 1, i, q.breg, breg, q.breg);
                a_changes += 1, b_changes += q.breg != breg, both += q.breg != breg;
            }
            super.push_back(Step{i, p.nt, p.mt, breg});
        }
        for (int nt = 0; nt < mo::NT; nt++)
            for (int mt = 0; mt < mt_tiles; mt++)
                EXPECT(seen[nt * mt_tiles + mt] == (mt >= lo && mt < hi ? 1 : 0), "%s k-step %d: (%d, %d) appears %d times", name, i, nt, mt, seen[nt * mt_tiles + mt]);
        ascending_b_changes += n - (i == 0 ? 1 : 0);  // nt outer, mt ascending: B changes with every MFMA
    }
    // distance between two MFMAs into one accumulator, over two super-steps back to back
    std::vector<Step> two = super;
    two.insert(two.end(), super.begin(), super.end());
    int nearest = 1 << 30;
    for (size_t a = 0; a < two.size(); a++)
        for (size_t b = a + 1; b < two.size() && b <= a + 64; b++)
            if (two[a].nt == two[b].nt && two[a].mt == two[b].mt) {
                if ((int)(b - a) < nearest) nearest = (int)(b - a);
                break;
            }
    EXPECT(nearest > 4, "%s: an accumulator recurs after %d positions", name, nearest);
    std::printf("%s: %zu MFMAs per super-step; inside it A changes %d times, B %d times (ascending order: %d), both at once %d times; nearest reuse of an accumulator %d positions\n",
                name, super.size(), a_changes, b_changes, ascending_b_changes, both, nearest);
}

int main() {
    check("line tiles 1..7 / 0..7 / 0..6", mo::line_rows(8), 8);
    check("one row 0..7", mo::one_row(8), 8);
    // the seam rule itself: dy = 0 carries register 0 over from dy = -1, dy = +1 has no register 0 and starts at its low end
    const mo::Rows r = mo::line_rows(8);
    EXPECT(!mo::starts_high(r, 0) && !mo::starts_high(r, 1) && !mo::starts_high(r, 2), "the line tiles' k-steps all start at their low end");
    const mo::Pos last0 = mo::at(r, 0, mo::count(r, 0) - 1), first1 = mo::at(r, 1, 0);
    EXPECT(last0.mt + r.dy[0] == 0 && first1.mt + r.dy[1] == 0, "dy = -1 ends on register %d, dy = 0 starts on %d", last0.mt + r.dy[0], first1.mt + r.dy[1]);
    // and a case where the rule turns a k-step around: the second row's HIGH end has the register the first ended on
    const mo::Rows t{2, {0, 0, 0}, {4, 2, 0}, {0, -1, 0}};  // row 0 ends on register 0; row 1 reads registers -1..0: tile 1 has it
    EXPECT(mo::starts_high(t, 1) && mo::at(t, 1, 0).mt == 1, "a k-step starts at the end that carries the register");
    std::printf("tower mfma order tests %s, %d failures\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
