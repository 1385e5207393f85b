// A stand-alone program (its own main) over the host-buildable lane functions of csrc/ble_scenarios.h -- the scenario stream and the
// risk ranks and score -- for tests/test_scenario_host.py, which builds it with g++ -fsanitize=address,undefined and runs it as a child
// process.  TEST TOOLING, compiled with tests/emul/ble_intrinsics.h force-included as tests/replay_draws.cpp is.  It checks what a
// sanitizer cannot: the two ways to the harmonic words agree, ranks are a permutation, the score is the plain ordered mean.
#include <stdio.h>
#include <stdlib.h>

#include "../balloon_learning_environment_amd/csrc/ble_scenarios.h"

using namespace ble;

static int fail(const char* what, long long a, long long b) {
  printf("FAILED %s at %lld, %lld\n", what, a, b);
  return 1;
}

int main() {
  // ---- the stream: every scenario of a few (seed, key, episode), in order and harmonic by harmonic, exactly 50 words each
  const uint64_t seeds[] = {0ull, 1ull, 0x5EEDF00Dull, 0xFFFFFFFFFFFFFFFFull, 0x0123456789ABCDEFull};
  uint64_t sum = 0;
  for (int si = 0; si < 5; ++si) {
    for (uint64_t key = 0; key < 3; ++key) {
      uint32_t truth[50];
      noise_draws_fetch(seeds[si], 0, key * 0x100000001ull, 7u, nullptr, 1, truth, 1);
      for (int m = 0; m < kScenarioMax; ++m) {
        uint32_t* words = (uint32_t*)malloc(50 * sizeof(uint32_t));      // (heap: one word past the end is the sanitizer's to catch)
        scenario_draws_fetch(seeds[si], key * 0x100000001ull, 7u, m, words, 1);
        for (int k = 0; k < 10; ++k) {
          const HarmonicDraw d = scenario_harmonic(seeds[si], key * 0x100000001ull, 7u, m, k);
          const uint32_t w[5] = {d.hseed, float_bits_u32(d.ox), float_bits_u32(d.oy), float_bits_u32(d.op), float_bits_u32(d.ot)};
          for (int r = 0; r < 5; ++r)
            if (w[r] != words[5 * k + r]) return fail("scenario_harmonic vs scenario_draws_fetch", m, 5 * k + r);
          if (!(d.ox >= -1.0f && d.ox <= 1.0f && d.ot >= -1.0f && d.ot <= 1.0f)) return fail("offset range", m, k);
        }
        int same = 0;
        for (int r = 0; r < 50; ++r) { same += words[r] == truth[r]; sum += words[r]; }
        if (same > 2) return fail("a scenario repeats the truth's words", m, same);
        free(words);
      }
    }
  }
  // ---- the risk score: every M and tail over crafted returns (ties, signed zeros, a NaN, an Inf), strided and dense
  const float nan = __builtin_nanf(""), inf = __builtin_inff();
  for (int num = 1; num <= kScenarioMax; ++num) {
    float* ret = (float*)malloc(3 * num * sizeof(float));
    for (int variant = 0; variant < 4; ++variant) {
      for (int m = 0; m < num; ++m) {
        float v = (float)((m * 7 + 3) % 5) - 2.0f;                      // ties among -2 .. 2
        if (v == 0.0f && (m & 1)) v = -0.0f;
        if (variant == 1 && m == num / 2) v = nan;
        if (variant == 2 && m == num - 1) v = -inf;
        if (variant == 3) v = 0.25f * (float)(num - m);                  // strictly descending: rank = num - 1 - m
        ret[3 * m] = v; ret[3 * m + 1] = 1e30f; ret[3 * m + 2] = nan;     // (stride 3: the neighbours must never be read)
      }
      const uint64_t ranks = risk_ranks(ret, 3, num);
      unsigned seen = 0;
      for (int m = 0; m < num; ++m) seen |= 1u << ((ranks >> (4 * m)) & 15u);
      if (variant != 1 && seen != (num == 32 ? ~0u : (1u << num) - 1u)) return fail("ranks are no permutation", num, variant);
      for (int tail = 1; tail <= num; ++tail) {
        const float score = plan_risk_score(ret, 3, num, tail);
        if (variant == 1 || variant == 2) {
          if (score == score) return fail("a non-finite return must score NaN", num, tail);
          continue;
        }
        if (variant == 3) {                                              // the tail smallest are the last `tail` entries, ascending from the end
          double s = 0.0;
          for (int r = 0; r < tail; ++r) s += (double)ret[3 * (num - 1 - r)];
          if (score != (float)(s / (double)tail)) return fail("score of a descending row", num, tail);
        }
        if (!(score >= -2.0f && score <= 0.25f * (float)num + 2.0f)) return fail("score out of the returns' range", num, tail);
      }
    }
    free(ret);
  }
  printf("ok %llu\n", (unsigned long long)(sum & 0xFFFFull));
  return 0;
}
