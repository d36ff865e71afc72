// Exhaustive check behind blur_large_u8.hip box_large_kernel (verification aid, not product code):
// for every odd window side k = 3 .. 31 and every window sum S = 0 .. 255 k^2 the box filter's
// result (2 S + k^2) / (2 k^2) equals the high word of (S + (k^2 - 1) / 2) * M with
// M = floor(2^32 / k^2) + 1, the one multiply the kernel does (__umulhi), and lies in 0 .. 255.
//   gcc -O2 -o /tmp/check_blur_div tools/check_blur_div.c
//   /tmp/check_blur_div        (about 1.4e6 quotients)
#include <stdint.h>
#include <stdio.h>
int main(void) {
  long long bad = 0, tot = 0;
  for (uint32_t k = 3; k <= 31; k += 2) {
    const uint32_t k2 = k * k, half = (k2 - 1) / 2;
    const uint32_t magic = (uint32_t)((1ull << 32) / k2 + 1);
    for (uint32_t s = 0; s <= 255u * k2; ++s) {
      const uint32_t want = (2 * s + k2) / (2 * k2);
      const uint32_t got = (uint32_t)(((uint64_t)(s + half) * magic) >> 32);
      tot++;
      if (got != want || got > 255) {
        if (bad < 5) printf("mismatch k=%u s=%u want=%u got=%u\n", k, s, want, got);
        bad++;
      }
    }
  }
  printf("checked %lld, mismatches %lld\n", tot, bad);
  return bad != 0;
}
