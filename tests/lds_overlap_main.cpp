// The biased packed deltas of the shaped row loop of k_lds2opt on the CPU (csrc/tspgpu_lds_tmat.h: pk_bias, pk_biased, PK_BIAS;
// csrc/tspgpu_lds2opt.inc: the row loop).  Stand-alone, built with AddressSanitizer and UBSan by
// tests/test_lds_overlap_model.py; prints "lds_overlap ok".
//   x + y + (0x8000 - w[k]) - w[m] in unsigned 16-bit halves of one 32-bit sum, XOR 0x8000, is the signed delta of the unbiased
//   form, half by half; no carry crosses the halves; the unsigned order of the biased halves is the signed order of the deltas
#include <cstdio>
#include <cstdlib>

#include "tspgpu_lds_tmat.h"

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }

static void bias_of(unsigned x0, unsigned y0, unsigned x1, unsigned y1, unsigned wk, unsigned wm0, unsigned wm1)
{
    const unsigned X = x0 | x1 << 16, Y = y0 | y1 << 16;
    const unsigned b = lds_tmat::pk_bias(wk);
    CHECK((b & 0xffffu) == 0x8000u - wk && (b >> 16) == 0x8000u - wk, "wk %u", wk);
    const unsigned s = lds_tmat::pk_biased(X, Y, b);
    const unsigned h0 = x0 + y0 + 0x8000u - wk, h1 = x1 + y1 + 0x8000u - wk;
    CHECK(h0 >= 16385u && h0 <= 65534u && h1 >= 16385u && h1 <= 65534u, "a half leaves [16385, 65534]: %u %u", h0, h1);
    CHECK((s & 0xffffu) == h0 && (s >> 16) == h1, "a carry crossed the halves: x %u %u y %u %u wk %u", x0, x1, y0, y1, wk);
    // - w[m] half by half, then the bias off: the signed 16-bit deltas of the unbiased form
    const unsigned p = (((s & 0xffffu) - wm0) & 0xffffu) | (((s >> 16) - wm1) & 0xffffu) << 16;
    CHECK((p & 0xffffu) >= 2u && (p & 0xffffu) <= 65534u && (p >> 16) >= 2u && (p >> 16) <= 65534u, "a half leaves [2, 65534]");
    const unsigned d = p ^ lds_tmat::PK_BIAS;
    const int want0 = (int)x0 + (int)y0 - (int)wk - (int)wm0, want1 = (int)x1 + (int)y1 - (int)wk - (int)wm1;
    CHECK((int)(short)(d & 0xffffu) == want0 && (int)(short)(d >> 16) == want1, "x %u %u y %u %u wk %u wm %u %u: %d %d, not %d %d", x0, x1, y0, y1, wk, wm0, wm1,
          (int)(short)(d & 0xffffu), (int)(short)(d >> 16), want0, want1);
}

static void bias()
{
    const unsigned v[6] = {0, 1, 2, 8190, 16382, 16383};
    for (unsigned x : v) for (unsigned y : v) for (unsigned wk : v) for (unsigned wm : v) {
        bias_of(x, y, x, y, wk, wm, wm);
        bias_of(x, y, 16383 - x, 16383 - y, wk, wm, 16383 - wm);      // (the other half at the other end)
        bias_of(16383 - x, y, x, 16383 - y, wk, 16383 - wm, wm);
    }
    unsigned prev = 0, prev_key = 0;
    for (int i = 0; i < 1000000; i++) {
        const unsigned x0 = rnd() % 16384, y0 = rnd() % 16384, x1 = rnd() % 16384, y1 = rnd() % 16384, wk = rnd() % 16384;
        bias_of(x0, y0, x1, y1, wk, rnd() % 16384, rnd() % 16384);
        // the order: the unsigned minimum of two biased halves picks what the signed minimum of the two deltas picks
        const unsigned h = x0 + y0 + 0x8000u - wk;
        const int dl = (int)x0 + (int)y0 - (int)wk;
        if (i) CHECK((h < prev) == (dl < (int)prev_key - 0x8000) && (h == prev) == (dl == (int)prev_key - 0x8000), "the biased order is not the signed order");
        prev = h; prev_key = h;
    }
}

int main()
{
    bias();
    std::printf("lds_overlap ok\n");
    return 0;
}
