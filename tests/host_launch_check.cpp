// Stand-alone check of the plain host helpers of csrc/tt_host.h: the precision dispatch, the flag -> mode maps and the
// grid of the queue-driven kernels.  Makes no HIP call and loads no library; built and run by tests/test_host_logic.py.
#include <stdio.h>

#include "../triplaneturbo_amd/csrc/tt_host.h"

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            ++failures;                       \
            printf("FAILED %s: ", #cond);     \
            printf(__VA_ARGS__);              \
            printf("\n");                     \
        }                                     \
    } while (0)

int main() {
    // the dispatcher hands over exactly the constants asked for, once
    const int precs[3] = {PREC_S2, PREC_F32, PREC_S3};
    for (int prec : precs) {
        int calls = 0, got = -1;
        tt_dispatch_prec(prec, [&](auto P) {
            ++calls;
            got = decltype(P)::value;
        });
        CHECK(calls == 1 && got == prec, "tt_dispatch_prec(%d): %d call(s), PREC %d", prec, calls, got);
        for (int n = 0; n < 2; ++n)
            for (int t = 0; t < 2; ++t) {
                int gp = -1, gn = -1, gt = -1;
                calls = 0;
                tt_dispatch(prec, n != 0, t != 0, [&](auto P, auto N, auto T) {
                    ++calls;
                    gp = decltype(P)::value;
                    gn = decltype(N)::value;
                    gt = decltype(T)::value;
                });
                CHECK(calls == 1 && gp == prec && gn == n && gt == t, "tt_dispatch(%d, %d, %d): %d call(s), got (%d, %d, %d)",
                      prec, n, t, calls, gp, gn, gt);
            }
    }
    CHECK(PREC_S2 != PREC_F32 && PREC_S2 != PREC_S3 && PREC_F32 != PREC_S3, "the three modes are distinct");

    // flag word -> mode (tt_abi.h): no precision bit = three-piece split (default), SPLIT2 = fast, EXACT_F32 = fp32 MFMA;
    // the other bits of the word do not matter
    for (int other = 0; other < 2; ++other) {
        const int r = other ? (TT_R_PER_SAMPLE | TT_R_VOLSDF | TT_R_BWD_SOLO) : 0, q = other ? (TT_Q_NORMAL | TT_Q_TEX) : 0;
        CHECK(tt_prec_of_r(r) == PREC_S3 && tt_prec_of_r(r | TT_R_SPLIT3) == PREC_S3, "render flags %d: default", r);
        CHECK(tt_prec_of_r(r | TT_R_SPLIT2) == PREC_S2, "render flags %d: SPLIT2", r);
        CHECK(tt_prec_of_r(r | TT_R_EXACT_F32) == PREC_F32, "render flags %d: EXACT_F32", r);
        CHECK(tt_prec_of_q(q) == PREC_S3 && tt_prec_of_q(q | TT_Q_SPLIT3) == PREC_S3, "query flags %d: default", q);
        CHECK(tt_prec_of_q(q | TT_Q_SPLIT2) == PREC_S2, "query flags %d: SPLIT2", q);
        CHECK(tt_prec_of_q(q | TT_Q_EXACT_F32) == PREC_F32, "query flags %d: EXACT_F32", q);
        CHECK(tt_qflags_ok(q) && tt_qflags_ok(q | TT_Q_SPLIT2) && tt_qflags_ok(q | TT_Q_SPLIT3) && tt_qflags_ok(q | TT_Q_EXACT_F32),
              "query flags %d: one precision bit is fine", q);
        CHECK(!tt_qflags_ok(q | TT_Q_SPLIT2 | TT_Q_EXACT_F32) && !tt_qflags_ok(q | TT_Q_SPLIT2 | TT_Q_SPLIT3) &&
                  !tt_qflags_ok(q | TT_Q_SPLIT3 | TT_Q_EXACT_F32),
              "query flags %d: two precision bits are not", q);
    }

    // grid of a queue-driven kernel, against the formula every entry point spelled out before they shared one:
    // min(cus, ceil(n_items / waves)), rounded up to a multiple of 8
    const int cus_list[5] = {1, 8, 255, 256, 304}, waves_list[2] = {4, 8};
    for (int cus : cus_list)
        for (int waves : waves_list)
            for (long long k = 1; k <= 4097; ++k) {
                const long long n_items = k <= 4096 ? k : (1LL << 30);
                long long want = cus;
                const long long need = (n_items + waves - 1) / waves;
                if (want > need) want = need;
                want = (want + 7) / 8 * 8;
                const long long got = tt_persistent_blocks(n_items, cus, waves);
                CHECK(got == want, "tt_persistent_blocks(%lld, %d, %d) = %lld, want %lld", n_items, cus, waves, got, want);
            }
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
