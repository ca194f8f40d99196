// test_stream_shift.cpp — kz::stream_shift (kzero_amd/csrc/kz_model.cpp) on the host, under the address and undefined-behaviour
// sanitizers: links the host model code only.  usage: test_stream_shift <model.kzm>...
//
// Every shifted tensor equals ldexpf(source, -+k) bit for bit, every other tensor and the descriptor are untouched,
// shift(shift(m, -12), 12) is m bit for bit, and a value that would leave f32's normal range is refused.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../kzero_amd/csrc/kz_model.hpp"

using kz::Model;

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            failures++;                                    \
            printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                           \
            printf("\n");                                  \
        }                                                  \
    } while (0)

typedef std::vector<std::pair<std::string, const std::vector<float> *>> Tensors;

static void add(Tensors &t, const std::string &name, const kz::Conv &c) {
    t.push_back({name + ".w", &c.w});
    t.push_back({name + ".b", &c.b});
}
static void add(Tensors &t, const std::string &name, const kz::Linear &l) {
    t.push_back({name + ".w", &l.w});
    t.push_back({name + ".b", &l.b});
}

// every float tensor of a model, by name
static Tensors tensors(const Model &m) {
    Tensors t;
    for (size_t i = 0; i < m.tower.size(); i++) add(t, "tower." + std::to_string(i), m.tower[i]);
    t.push_back({"final_scale", &m.final_scale});
    t.push_back({"final_shift", &m.final_shift});
    t.push_back({"att_expand", &m.att_expand});
    t.push_back({"att_embedding", &m.att_embedding});
    for (size_t i = 0; i < m.att_layers.size(); i++) {
        const std::string p = "att." + std::to_string(i);
        t.push_back({p + ".qkv", &m.att_layers[i].qkv});
        t.push_back({p + ".out", &m.att_layers[i].out});
        t.push_back({p + ".ff0", &m.att_layers[i].ff0});
        t.push_back({p + ".ff1", &m.att_layers[i].ff1});
    }
    add(t, "sh_conv", m.sh_conv);
    add(t, "sh_fc0", m.sh_fc0);
    add(t, "sh_fc1", m.sh_fc1);
    add(t, "p_conv0", m.p_conv0);
    add(t, "p_conv1", m.p_conv1);
    add(t, "p_extra_conv", m.p_extra_conv);
    add(t, "p_extra_fc", m.p_extra_fc);
    add(t, "p_bulk", m.p_bulk);
    add(t, "p_under", m.p_under);
    add(t, "p_fc0", m.p_fc0);
    add(t, "p_fc1", m.p_fc1);
    add(t, "pa_conv", m.pa_conv);
    add(t, "pa_fc0", m.pa_fc0);
    add(t, "pa_fc1", m.pa_fc1);
    add(t, "dn_in", m.dn_in);
    add(t, "dn_out", m.dn_out);
    t.push_back({"dn_sf", &m.dn_sf});
    t.push_back({"dn_tf", &m.dn_tf});
    return t;
}

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * 4) == 0);
}

// the exponent a tensor of the shifted model carries against the source's: -k, +k, or 0 (untouched)
static int exponent_of(const std::string &name, int k) {
    if (name == "tower.0.w") return -k;
    if (name.rfind("tower.", 0) == 0 && name.size() > 2 && name.compare(name.size() - 2, 2, ".b") == 0) return -k;
    if (name == "final_scale") return k;
    return 0;
}

static void same_descriptor(const Model &a, const Model &b) {
    CHECK(a.game == b.game && a.h == b.h && a.w == b.w && a.n_scalar == b.n_scalar && a.n_bool == b.n_bool && a.c_in == b.c_in, "board");
    CHECK(a.depth == b.depth && a.channels == b.channels && a.policy_len == b.policy_len && a.policy_kind == b.policy_kind, "tower / policy");
    CHECK(a.policy_conv_channels == b.policy_conv_channels && a.policy_extra_moves == b.policy_extra_moves &&
              a.policy_query_channels == b.policy_query_channels && a.dense_hidden_channels == b.dense_hidden_channels &&
              a.dense_hidden_size == b.dense_hidden_size, "policy head");
    CHECK(a.tower_kind == b.tower_kind && a.flat_to_att == b.flat_to_att, "tower kind / attention map");
    CHECK(a.param_count == b.param_count && a.flops_per_eval == b.flops_per_eval, "counts");
    CHECK(a.tower.size() == b.tower.size(), "tower size");
    for (size_t i = 0; i < a.tower.size() && i < b.tower.size(); i++)
        CHECK(a.tower[i].cout == b.tower[i].cout && a.tower[i].cin == b.tower[i].cin && a.tower[i].k == b.tower[i].k, "conv %zu", i);
}

static void check_shift(const Model &m, int k) {
    std::string err;
    std::unique_ptr<Model> s(kz::stream_shift(m, k, err));
    CHECK(s != nullptr, "k = %d refused: %s", k, err.c_str());
    if (!s) return;
    same_descriptor(m, *s);
    const Tensors src = tensors(m), dst = tensors(*s);
    CHECK(src.size() == dst.size(), "tensor count");
    size_t moved = 0;
    for (size_t t = 0; t < src.size() && t < dst.size(); t++) {
        const std::vector<float> &a = *src[t].second, &b = *dst[t].second;
        const int e = exponent_of(src[t].first, k);
        CHECK(a.size() == b.size(), "%s: size", src[t].first.c_str());
        if (a.size() != b.size()) continue;
        CHECK(a.data() != b.data() || a.empty(), "%s: the shifted model shares storage with its source", src[t].first.c_str());
        if (e == 0) {
            CHECK(same_bits(a, b), "%s: changed by k = %d", src[t].first.c_str(), k);
            continue;
        }
        moved++;
        size_t bad = 0;
        for (size_t i = 0; i < a.size(); i++) {
            const float want = ldexpf(a[i], e);
            bad += memcmp(&want, &b[i], 4) != 0;
        }
        CHECK(bad == 0, "%s: %zu of %zu values differ from ldexpf(source, %d)", src[t].first.c_str(), bad, a.size(), e);
    }
    // the stem's weights, 2 * depth + 1 biases, the final scale
    CHECK(moved == (k ? (size_t)(2 * m.depth + 3) : 0), "k = %d: %zu tensors moved, %d expected", k, moved, k ? 2 * m.depth + 3 : 0);
}

static void check_round_trip(const Model &m) {
    std::string err;
    std::unique_ptr<Model> up(kz::stream_shift(m, -12, err));
    CHECK(up != nullptr, "%s", err.c_str());
    if (!up) return;
    std::unique_ptr<Model> back(kz::stream_shift(*up, 12, err));
    CHECK(back != nullptr, "%s", err.c_str());
    if (!back) return;
    same_descriptor(m, *back);
    const Tensors a = tensors(m), b = tensors(*back);
    for (size_t t = 0; t < a.size(); t++) CHECK(same_bits(*a[t].second, *b[t].second), "%s: not the source's bits after -12, +12", a[t].first.c_str());
    // and a copy is a copy
    std::unique_ptr<Model> copy(kz::stream_shift(m, 0, err));
    CHECK(copy != nullptr, "%s", err.c_str());
    if (!copy) return;
    const Tensors c = tensors(*copy);
    for (size_t t = 0; t < a.size(); t++) CHECK(same_bits(*a[t].second, *c[t].second), "%s: k = 0 changed it", a[t].first.c_str());
}

static std::string refused(const Model &m, int k) {
    std::string err;
    std::unique_ptr<Model> s(kz::stream_shift(m, k, err));
    CHECK(s == nullptr, "k = %d accepted", k);
    CHECK(!err.empty(), "k = %d: refused without a message", k);
    return err;
}

static void check_refusals(const Model &m) {
    std::vector<std::string> messages;
    messages.push_back(refused(m, 25));
    messages.push_back(refused(m, -25));
    {
        Model a(m);
        a.tower_kind = kz::TOWER_ATTENTION;
        messages.push_back(refused(a, 1));
        a.tower_kind = kz::TOWER_DENSE_NET;
        messages.push_back(refused(a, 1));
    }
    {
        Model a(m);
        a.depth = 0;
        a.tower.resize(1);
        messages.push_back(refused(a, 1));
    }
    // a value that would go subnormal: 2^-120 * 2^-12 (nothing rounds silently); its neighbours do not matter
    for (int where = 0; where < 3; where++) {
        Model a(m);
        float &v = where == 0 ? a.tower[0].w[a.tower[0].w.size() / 2] : where == 1 ? a.tower[1].b[0] : a.tower.back().b.back();
        v = ldexpf(where == 1 ? -1.5f : 1.0f, -120);
        const std::string e = refused(a, 12);
        CHECK(e.find("normal range") != std::string::npos, "subnormal (%d): %s", where, e.c_str());
        if (where == 0) messages.push_back(e);
        std::string err;
        std::unique_ptr<Model> ok(kz::stream_shift(a, 6, err));  // 2^-126 is f32's smallest normal number: still exact
        CHECK(ok != nullptr, "2^-126 refused: %s", err.c_str());
        std::unique_ptr<Model> under(kz::stream_shift(a, 7, err));
        CHECK(under == nullptr, "2^-127 accepted");
    }
    {  // ... or overflow: the final scale goes the other way
        Model a(m);
        a.final_scale[a.final_scale.size() / 2] = ldexpf(-1.0f, 120);
        const std::string e = refused(a, 12);
        CHECK(e.find("normal range") != std::string::npos, "overflow: %s", e.c_str());
        std::string err;
        std::unique_ptr<Model> ok(kz::stream_shift(a, 7, err));
        CHECK(ok != nullptr, "2^127 refused: %s", err.c_str());
        std::unique_ptr<Model> down(kz::stream_shift(a, -12, err));
        CHECK(down != nullptr, "the scale shrinks with a negative k: %s", err.c_str());
    }
    {  // zeros stay zeros and are never a reason to refuse
        Model a(m);
        a.tower[1].b[0] = 0.0f;
        a.tower[0].w[0] = -0.0f;
        std::string err;
        std::unique_ptr<Model> s(kz::stream_shift(a, 24, err));
        CHECK(s != nullptr, "%s", err.c_str());
        if (s) CHECK(s->tower[1].b[0] == 0.0f && s->tower[0].w[0] == 0.0f && std::signbit(s->tower[0].w[0]), "zeros");
    }
    for (size_t i = 0; i < messages.size(); i++)
        for (size_t j = i + 1; j < messages.size(); j++)
            if (!(i == 0 && j == 1)) CHECK(messages[i] != messages[j], "two refusals share a message: %s", messages[i].c_str());
}

int main(int argc, char **argv) {
    if (argc < 2) {
        printf("usage: test_stream_shift <model.kzm>...\n");
        return 2;
    }
    for (int f = 1; f < argc; f++) {
        std::vector<uint8_t> blob;
        FILE *fp = fopen(argv[f], "rb");
        if (!fp) {
            printf("cannot open %s\n", argv[f]);
            return 2;
        }
        uint8_t tmp[1 << 16];
        size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, fp)) > 0) blob.insert(blob.end(), tmp, tmp + n);
        fclose(fp);
        std::string err;
        std::unique_ptr<Model> m(kz::parse_model(blob.data(), blob.size(), err));
        if (!m) {
            printf("%s: %s\n", argv[f], err.c_str());
            return 2;
        }
        for (int k : {3, 12, -12, 24, -24, 1, 0}) check_shift(*m, k);
        check_round_trip(*m);
        check_refusals(*m);
        printf("%s: depth %d, %d channels: checked\n", argv[f], m->depth, m->channels);
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("stream shift tests ok\n");
    return 0;
}
