/* lift_range_check.c -- TEST INFRASTRUCTURE, CPU only.
 *
 * A stand-alone program around oracle/lift_oracle.c, compiled with
 * -fsanitize=signed-integer-overflow -fno-sanitize-recover=all
 * (tests/lift_edge_cases.py: build_range_check): it runs one forward lifting case
 * read from a file of raw arrays and ends abnormally when a signed product of the
 * reference's arithmetic (`scaled * iQuantWeight` above all) leaves 64 bits, i.e.
 * when the case is outside the range in which the reference's result is defined.
 *
 *   lift_range_check CASE [OUT]
 *
 * CASE: int32 {n, c, has_qp_off}, gpcc_lift_params, neigh_count [n], neigh_index
 * [n][3], neigh_weight [n][3], indexes [n], qp_off [n][2] when has_qp_off, attrs
 * [n][c] -- all int32.  OUT (optional): coeffs [n][c], recon [n][c] as int32 and
 * the 32 last-component coefficients.  Exit 0: inside the exact range. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "gpcc_attr_mi355.h"

int oracle_lift_forward(
  const gpcc_lift_params*, int32_t, int32_t, const int32_t*, const int32_t*, const int32_t*, const int32_t*,
  const int32_t*, int32_t*, int32_t*, int8_t*);

static int
get(void* dst, size_t size, size_t count, FILE* f)
{
  return fread(dst, size, count, f) == count;
}

int
main(int argc, char** argv)
{
  if (argc < 2)
    return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f)
    return 2;
  int32_t hdr[3];
  gpcc_lift_params p;
  if (!get(hdr, 4, 3, f) || !get(&p, sizeof p, 1, f))
    return 2;
  const int32_t n = hdr[0], c = hdr[1], has_q = hdr[2];
  if (n <= 0 || n > (1 << 24) || c < 1 || c > 3)
    return 2;
  const size_t N = (size_t)n;
  int32_t* nc = malloc(4 * N);
  int32_t* ni = malloc(12 * N);
  int32_t* nw = malloc(12 * N);
  int32_t* idx = malloc(4 * N);
  int32_t* q = malloc(8 * N);
  int32_t* a = malloc(4 * N * c);
  int32_t* co = calloc(N * c, 4);
  if (!nc || !ni || !nw || !idx || !q || !a || !co)
    return 2;
  if (!get(nc, 4, N, f) || !get(ni, 4, 3 * N, f) || !get(nw, 4, 3 * N, f) || !get(idx, 4, N, f)
      || (has_q && !get(q, 4, 2 * N, f)) || !get(a, 4, N * c, f))
    return 2;
  fclose(f);
  int8_t lcp[GPCC_MAX_LODS] = {0};
  const int rc = oracle_lift_forward(&p, n, c, nc, ni, nw, idx, has_q ? q : NULL, a, co, lcp);
  if (rc)
    return 3;
  if (argc > 2) {
    FILE* o = fopen(argv[2], "wb");
    if (!o)
      return 2;
    fwrite(co, 4, N * c, o);
    fwrite(a, 4, N * c, o);
    fwrite(lcp, 1, sizeof lcp, o);
    fclose(o);
  }
  return 0;
}
