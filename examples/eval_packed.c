/* examples/eval_packed.c — the C ABI of include/kz_hip.h from plain C (what any FFI sees): load a model, create an
 * engine, evaluate a batch of packed boards, read the results in place, clean up.  Every call returns 0 or sets
 * kz_last_error().
 *
 *   gcc -std=c99 -I include examples/eval_packed.c -L kzero_amd -lkzhip -Wl,-rpath,$PWD/kzero_amd -o /tmp/eval_packed
 *   /tmp/eval_packed tests/golden/ataxx7_4x64.kzm
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kz_hip.h"

#define CHECK(call)                                                      \
    do {                                                                 \
        if ((call) != 0) {                                               \
            fprintf(stderr, "%s failed: %s\n", #call, kz_last_error()); \
            return 1;                                                    \
        }                                                                \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s model.kzm|model.onnx [input_scalar_channels for ONNX]\n", argv[0]);
        return 2;
    }
    kz_model *model = NULL;
    const size_t n = strlen(argv[1]);
    if (n > 5 && strcmp(argv[1] + n - 5, ".onnx") == 0) CHECK(kz_model_load_onnx(argv[1], argc > 2 ? atoi(argv[2]) : 0, &model));
    else CHECK(kz_model_load(argv[1], &model));
    kz_model_info info;
    CHECK(kz_model_get_info(model, &info));
    printf("model: %d planes (%d scalar + %d bool) on %dx%d, tower %dx%d, policy %d\n", info.input_channels,
           info.input_scalar_channels, info.input_bool_channels, info.board_h, info.board_w, info.tower_depth,
           info.tower_channels, info.policy_len);

    const int batch = 4;
    kz_engine *engine = NULL;
    CHECK(kz_engine_create(model, 0, batch, KZ_DTYPE_F32, &engine));

    /* packed boards: BitBuffer storage (bit i of the bool planes = bit i%8 of byte i/8) + the scalar planes' values */
    unsigned char *bits = calloc((size_t)batch, (size_t)info.bits_bytes);
    float *scalars_in = calloc((size_t)batch * (size_t)(info.input_scalar_channels ? info.input_scalar_channels : 1), sizeof(float));
    for (int b = 0; b < batch; b++) bits[(size_t)b * info.bits_bytes] = (unsigned char)(1u << b); /* one piece each */

    /* asynchronous pair + zero-copy view; kz_engine_eval_packed is the one-call form with caller buffers */
    CHECK(kz_engine_submit_packed(engine, 0, bits, (size_t)info.bits_bytes, scalars_in, batch));
    const float *scalars_out = NULL, *policy = NULL;
    CHECK(kz_engine_wait_view(engine, 0, &scalars_out, &policy));
    for (int b = 0; b < batch; b++)
        printf("board %d: value logit %+.4f  wdl logits %+.4f %+.4f %+.4f  moves left %+.4f  policy[0] %+.4f\n", b,
               scalars_out[b * 5], scalars_out[b * 5 + 1], scalars_out[b * 5 + 2], scalars_out[b * 5 + 3],
               scalars_out[b * 5 + 4], policy[(size_t)b * info.policy_len]);

    /* decoded output with a status per board instead of a failing batch: two moves per board; board 1 lists a move index
     * outside the policy, so it comes back as KZ_BOARD_BAD_DECODE and the other boards' results stand.  (An f16 / split16
     * engine after kz_engine_set_range_fallback(engine, KZ_DTYPE_F32) reports a board it re-evaluated in exact f32 as
     * KZ_BOARD_FELL_BACK.) */
    /* ... and, beside it, the shadow audit: the batch's boards also run on a sibling engine in another <= 1e-4 arithmetic and
     * the engine accumulates how far the two are apart (this engine is exact f32, so the sibling is the split-f16 one; an f16
     * engine would be audited against KZ_DTYPE_F32_SPLIT16 or KZ_DTYPE_F32 the same way).  Nothing of the batch changes. */
    const int audited = kz_model_supports_dtype(model, KZ_DTYPE_F32_SPLIT16) == 1;
    if (audited) CHECK(kz_engine_set_audit(engine, KZ_DTYPE_F32_SPLIT16, 1, batch));
    int64_t move_offsets[5] = {0, 2, 4, 6, 8};
    int32_t move_indices[8] = {0, 1, 0, 1, 0, 1, 0, 1};
    move_indices[3] = info.policy_len;
    float values[4 * 5], probs[8];
    uint8_t status[4];
    CHECK(kz_engine_eval_packed_decoded_status(engine, bits, (size_t)info.bits_bytes, scalars_in, batch, NULL, move_offsets,
                                               move_indices, values, probs, status));
    for (int b = 0; b < batch; b++) {
        if (status[b] == KZ_BOARD_OK || status[b] == KZ_BOARD_FELL_BACK)
            printf("board %d: status %d  value %+.4f  p(move 0) %.4f  p(move 1) %.4f\n", b, status[b], values[b * 5], probs[2 * b], probs[2 * b + 1]);
        else
            printf("board %d: status %d (its results are unspecified)\n", b, status[b]);
    }

    if (audited) {
        kz_audit_stats audit;
        CHECK(kz_engine_audit_stats(engine, &audit, 0));
        printf("audit against split16: %lld boards compared, %lld skipped, max |dp| %.3g\n", (long long)audit.boards,
               (long long)audit.skipped, audit.max_abs_prob);
    }

    /* how much f16 headroom this network has on these boards, and the same function with a smaller residual stream: the
     * range profile measures max |x| per stored tower tensor in exact f32; k = max(0, ceil(log2(m / 65504)) + 2 bits of
     * headroom), m the maximum over the sites a shift moves (all but the last); the shifted model is an ordinary kz_model.
     * (ResTower networks with at least one block; the three calls fail with a message for the others.) */
    int n_sites = 0;
    if (kz_model_range_sites(model, &n_sites) == 0 && n_sites <= 64) {
        float site_max[64], board_max[4], m = 0.0f;
        CHECK(kz_model_range_profile(model, 0, bits, (size_t)info.bits_bytes, scalars_in, batch, site_max, board_max));
        for (int s = 0; s < n_sites; s++) {
            char name[32];
            CHECK(kz_model_range_site_name(model, s, name, sizeof name));
            printf("site %-12s max |x| %.6g (%.3g of 65504)\n", name, site_max[s], site_max[s] / 65504.0);
            if (s < n_sites - 1 && site_max[s] > m) m = site_max[s];
        }
        int k = 2; /* the headroom; then ceil(log2(m / 65504)) without libm */
        for (float top = 65504.0f; top < m; top *= 2.0f) k++;
        for (float top = 32752.0f; top >= m && k > 0; top /= 2.0f) k--;
        kz_model *shifted = NULL;
        CHECK(kz_model_stream_shift(model, k, &shifted));
        printf("stream max %.6g: k = %d (with 2 bits of headroom); the shifted model is evaluated like any other\n", m, k);
        kz_model_free(shifted);
    }

    free(bits);
    free(scalars_in);
    kz_engine_destroy(engine);
    kz_model_free(model);
    return 0;
}
