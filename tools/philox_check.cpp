// Host-only check of ops/hip/attn_dropout.h against at::Philox4_32, and
// generator of tests/golden/attn_dropout_philox.json.
//
//   g++ -std=c++17 -I<torch>/include -Ialphafold2_amd/ops/hip \
//       tools/philox_check.cpp -o philox_check && ./philox_check > out.json
//
// 1. philox4x32_10(seed, subseq, offset) must equal the first four
//    outputs of at::Philox4_32(seed, subseq, offset) on a sweep that
//    crosses the 32-bit boundaries of seed, subsequence and offset.
// 2. Prints, as JSON, a few (seed, subseq, offset) -> words vectors and
//    one keep mask built from at::Philox4_32 alone by the definition in
//    docs/PARITY.md; the numpy reference of the tests is checked
//    against this file on any machine.
#include <ATen/core/PhiloxRNGEngine.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "attn_dropout.h"

static void engine_words(uint64_t seed, uint64_t subseq, uint64_t offset,
                         uint32_t out[4]) {
  at::Philox4_32 eng(seed, subseq, offset);
  for (int i = 0; i < 4; ++i) out[i] = eng();
}

int main() {
  const uint64_t seeds[] = {0ull, 1ull, 0xffffffffull, 0x100000000ull,
                            67280421310721ull, 0xdeadbeefcafef00dull};
  const uint64_t subs[] = {0ull, 1ull, 5ull, 0xffffffffull, 0x100000000ull,
                           0x123456789abcull};
  const uint64_t offs[] = {0ull, 4ull, 0xfffffffcull, 0x100000000ull,
                           0x100000004ull, 0x7fffffff00000000ull};
  long bad = 0, n = 0;
  std::printf("{\"vectors\": [");
  bool first = true;
  for (uint64_t seed : seeds)
    for (uint64_t sub : subs)
      for (uint64_t off : offs) {
        uint32_t ref[4];
        engine_words(seed, sub, off, ref);
        const attn_drop::U4 got = attn_drop::philox4x32_10(seed, sub, off);
        for (int i = 0; i < 4; ++i) bad += got.w[i] != ref[i];
        if (n % 7 == 0) {  // a spread subset goes into the fixture
          std::printf("%s\n [\"%llu\", \"%llu\", \"%llu\", [%u, %u, %u, %u]]",
                      first ? "" : ",", (unsigned long long)seed,
                      (unsigned long long)sub, (unsigned long long)off,
                      ref[0], ref[1], ref[2], ref[3]);
          first = false;
        }
        ++n;
      }
  std::printf("\n],\n");

  // one keep mask from the engine alone: (B*H, Lq, Lk) = (3, 10, 14),
  // offset above 2^32, p = 0.1 -> T = 26
  const uint64_t seed = 0x5eed5eed12345ull, offset = 0x100000008ull;
  const int BH = 3, Lq = 10, Lk = 14, T = 26;
  const int H4 = (Lq + 3) / 4, W4 = (Lk + 3) / 4;
  const attn_drop::Params par{seed, offset, (uint32_t)T, 0.f, H4, W4};
  std::printf("\"mask\": {\"seed\": \"%llu\", \"offset\": \"%llu\", "
              "\"BH\": %d, \"Lq\": %d, \"Lk\": %d, \"T\": %d, \"keep\": \"",
              (unsigned long long)seed, (unsigned long long)offset, BH, Lq,
              Lk, T);
  for (int bh = 0; bh < BH; ++bh)
    for (int i = 0; i < Lq; ++i)
      for (int j = 0; j < Lk; ++j) {
        uint32_t w[4];
        const uint64_t sub =
            ((uint64_t)bh * H4 + (i >> 2)) * W4 + (uint64_t)(j >> 2);
        engine_words(seed, sub, offset, w);
        const bool keep = ((w[i & 3] >> (8 * (j & 3))) & 0xff) >= (uint32_t)T;
        bad += keep != attn_drop::keep(par, bh, i, j);
        std::putchar(keep ? '1' : '0');
      }
  std::printf("\"},\n\"threshold\": {\"0.25\": %u, \"0.1\": %u, \"0.001\": %u, "
              "\"0.999\": %u}\n}\n",
              attn_drop::threshold(0.25), attn_drop::threshold(0.1),
              attn_drop::threshold(0.001), attn_drop::threshold(0.999));
  std::fprintf(stderr, "%ld vectors, %ld mismatches against at::Philox4_32\n",
               n, bad);
  return bad == 0 ? 0 : 1;
}
