// Exhaustive check behind wiener.hip wn_div (verification aid, not product code): the
// Markstein-corrected quotient q1 = fma(fma(-q0, n, s), r, q0), q0 = s*r, r = 1/n equals the IEEE
// quotient s/n for every window size n = kh*kw (kh, kw odd, 1..31) and every integer window sum
// s the filter can form, 0 .. n*255^2 (the sums of t are the subset 0 .. n*255).
//   gcc -O2 -ffp-contract=off -mfma -o /tmp/check_wiener_div tools/check_wiener_div.c -lm
//   /tmp/check_wiener_div        (about 2.3e9 quotients)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
int main(void) {
  static char seen[962];
  long long bad = 0, tot = 0;
  for (int kh = 1; kh <= 31; kh += 2)
    for (int kw = kh; kw <= 31; kw += 2) {
      const int n = kh * kw;
      if (seen[n]) continue;
      seen[n] = 1;
      const double dn = (double)n, r = 1.0 / dn;
      const uint32_t top = (uint32_t)n * 65025u;
      for (uint32_t s = 0; s <= top; ++s) {
        const double a = (double)s;
        const double q = a / dn;
        const double q0 = a * r;
        const double q1 = fma(fma(-q0, dn, a), r, q0);
        tot++;
        if (q1 != q) {
          if (bad < 5) printf("mismatch s=%u n=%d q=%.17g q1=%.17g\n", s, n, q, q1);
          bad++;
        }
      }
    }
  printf("checked %lld, mismatches %lld\n", tot, bad);
  return bad != 0;
}
