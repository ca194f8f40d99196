// test_symmetry_tables.cpp — CPU test of the symmetry tables the engine takes (host/symmetry.hpp: SymmetryTables, d4_tables):
// against the reference's own Ataxx tables (tests/golden/ataxx_symmetry.txt), against the host's board and move mapping
// (ataxx_map_tiles, AtaxxSymBoard::map), and the Go tables against their defining properties.  Built and run by
// tests/test_symmetry_tables.py;   test_symmetry_tables <golden dir>   or   test_symmetry_tables dump-go <size>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <sstream>
#include <string>

#include "../../kzero_amd/csrc/host/symmetry.hpp"

using namespace kz::host;

static int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                          \
        }                                                                        \
    } while (0)

static bool is_permutation_row(const SymmetryTables &t, int sym) {
    std::vector<char> seen(t.hw, 0);
    for (int s = 0; s < t.hw; s++) {
        const int32_t v = t.src(sym, s);
        if (v < 0 || v >= t.hw || seen[v]) return false;
        seen[v] = 1;
    }
    return true;
}

// d4_tables(AtaxxStdMapper(size)).policy_map == the reference's map_mv, all 7 sizes x 8 symmetries; square_src is the inverse
// of "where tile i lands" (the row's first `area` entries: the copy moves) and agrees with ataxx_map_tiles
static void test_ataxx_tables(const std::string &golden_dir) {
    std::ifstream f(golden_dir + "/ataxx_symmetry.txt");
    CHECK(f.good());
    std::string line;
    int rows = 0;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        int size, sym, tr, fx, fy;
        size_t n;
        is >> size >> sym >> tr >> fx >> fy >> n;
        const AtaxxStdMapper m(size);
        const SymmetryTables t = d4_tables(m);
        CHECK(t.n_sym == 8 && t.hw == size * size && (size_t)t.policy_len == n && n == m.policy_len());
        CHECK(t.square_src.size() == (size_t)8 * t.hw && t.policy_map.size() == (size_t)8 * n);
        bool same = true;
        std::vector<long> row(n);
        for (size_t i = 0; i < n; i++) {
            is >> row[i];
            same &= t.map(sym, i) == row[i];
        }
        CHECK(same);
        CHECK(is_permutation_row(t, sym));
        for (int i = 0; i < t.hw; i++) {
            CHECK(row[i] >= 0 && row[i] < t.hw && t.src(sym, (int)row[i]) == i);
            CHECK(ataxx_map_tiles(size, sym, 1ull << i) == 1ull << row[i]);
        }
        CHECK(t.map(sym, n - 1) == (int32_t)n - 1);  // pass stays pass
        rows++;
    }
    CHECK(rows == 7 * 8);
}

static void test_go_tables() {
    for (int size : {9, 19}) {
        const GoStdMapper m(size, true);
        const SymmetryTables t = d4_tables(m);
        const int area = size * size;
        CHECK(t.n_sym == 8 && t.hw == area && t.policy_len == 1 + area);
        for (int sym = 0; sym < 8; sym++) {
            CHECK(is_permutation_row(t, sym));
            CHECK(t.map(sym, 0) == 0);  // pass is fixed
            const D4 d = D4::from_index(sym);
            for (int s = 0; s < area; s++) {
                // the stone the mapped board has at s came from src(s): placing a stone there maps to placing one at s
                CHECK(t.map(sym, 1 + (size_t)t.src(sym, s)) == 1 + s);
                int x = t.src(sym, s) % size, y = t.src(sym, s) / size;
                d.map_xy(size, x, y);
                CHECK(y * size + x == s);
            }
            if (sym == 0)
                for (int s = 0; s < area; s++) CHECK(t.src(0, s) == s);
        }
        CHECK(t.src(4, 1) == size && t.src(2, 0) == size - 1 && t.src(1, 0) == area - size);  // transpose, flip x, flip y
    }
}

// applying the tables to a packed board == packing the mapped board; and the mapped board's move indices == policy_map of
// the board's own (as a set: AtaxxSymBoard::map sorts the mapped moves)
static void test_tables_against_board_map() {
    std::mt19937_64 rng(7);
    for (int size : {4, 7, 8}) {
        const AtaxxStdMapper m(size);
        const SymmetryTables t = d4_tables(m);
        const int area = size * size;
        const size_t bool_count = 3 * (size_t)area;
        for (int rep = 0; rep < 6; rep++) {
            AtaxxSymBoard b;
            b.size = size;
            for (int i = 0; i < area; i++) {
                const int r = (int)(rng() % 4);
                if (r == 0) b.tiles_next |= 1ull << i;
                if (r == 1) b.tiles_other |= 1ull << i;
                if (r == 2 && rng() % 2) b.gaps |= 1ull << i;
            }
            b.moves_since_last_copy = (int)(rng() % 100);
            std::vector<AtaxxMove> moves;
            for (int k = 0; k < 12; k++)
                if (auto mv = m.index_to_move(rng() % m.policy_len())) moves.push_back(*mv);
            b.moves = moves;
            BitBuffer own(bool_count);
            std::vector<float> scalars;
            m.encode_input(own, scalars, b);
            for (int sym = 0; sym < 8; sym++) {
                const AtaxxSymBoard mapped = b.map(sym);
                BitBuffer ref(bool_count);
                std::vector<float> mapped_scalars;
                m.encode_input(ref, mapped_scalars, mapped);
                CHECK(t.map_bits(sym, 3, own.storage()) == ref.storage());
                CHECK(mapped_scalars == scalars);  // scalar planes do not move
                std::vector<int32_t> via_table, via_board;
                for (const auto &mv : moves) via_table.push_back(t.map(sym, m.move_to_index(mv)));
                for (const auto &mv : *mapped.moves) via_board.push_back((int32_t)m.move_to_index(mv));
                std::sort(via_table.begin(), via_table.end());
                CHECK(via_table == via_board);
                for (const auto &mv : moves) CHECK(t.map(sym, m.move_to_index(mv)) == (int32_t)m.move_to_index(b.map_move(sym, mv)));
            }
        }
        // a jump whose source is off the board is no move under any symmetry
        size_t gone = 0;
        for (size_t i = 0; i < m.policy_len(); i++)
            if (!m.index_to_move(i)) {
                gone++;
                for (int sym = 0; sym < 8; sym++) CHECK(t.map(sym, i) == -1);
            } else {
                for (int sym = 0; sym < 8; sym++) CHECK(t.map(sym, i) >= 0 && t.map(sym, i) < t.policy_len);
            }
        CHECK(gone > 0);
    }
}

int main(int argc, char **argv) {
    if (argc > 2 && std::string(argv[1]) == "dump-go") {  // the tables as text, for the Python tests' own formula
        const SymmetryTables t = d4_tables(GoStdMapper(std::atoi(argv[2]), true));
        for (int sym = 0; sym < t.n_sym; sym++) {
            for (int s = 0; s < t.hw; s++) std::printf("%d ", t.src(sym, s));
            std::printf("|");
            for (int i = 0; i < t.policy_len; i++) std::printf(" %d", t.map(sym, (size_t)i));
            std::printf("\n");
        }
        return 0;
    }
    const std::string golden = argc > 1 ? argv[1] : "tests/golden";
    test_ataxx_tables(golden);
    test_go_tables();
    test_tables_against_board_map();
    if (g_failed) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    std::puts("symmetry table tests ok");
    return 0;
}
