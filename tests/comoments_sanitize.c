/* gel_batch_comoments* on a host-only handle under AddressSanitizer + UBSan (CPU build only; nothing is launched): every refusal of
 * both forms, decided before the device is looked at, what a valid call returns there, and gel_batch_comoments_info.  Prints
 * COMOMENTS_SANITIZE_OK on success. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/gelato_amd.h"

#define REQUIRE(c)                                                          \
  do {                                                                      \
    if (!(c)) { fprintf(stderr, "REQUIRE failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, gel_last_error()); return 1; } \
  } while (0)

typedef int (*comom_fn)(gel_problem*, int32_t, int64_t, int64_t, int64_t, const double*, int64_t, int64_t, int64_t, const double*, double*,
                        double*, double*, double*);

int main(void) {
  enum { S = 3 };
  const int32_t nn[S] = {2, 5, 3};
  const double thrust[S] = {420000.0, 0.0, 30700.0};
  const double mdot[S] = {140.0, 0.0, 9.8};
  const double area[S] = {2.21, 2.21, 0.0};
  const double nozzle[S] = {0.68, 0.0, 0.0};
  const int32_t on[S] = {1, 0, 1};
  const int32_t hold[S] = {1, 0, 0};
  const double wind[3][3] = {{0.0, 1.0, 2.0}, {5000.0, 3.0, -1.0}, {20000.0, 10.0, 4.0}};
  const double ca[2][2] = {{0.0, 0.3}, {5.0, 0.5}};
  gel_problem_desc d;
  memset(&d, 0, sizeof d);
  d.num_sections = S; d.num_nodes = nn; d.thrust = thrust; d.massflow = mdot; d.reference_area = area;
  d.nozzle_area = nozzle; d.engine_on = on; d.attitude_hold = hold;
  d.unit_mass = 27442.0; d.unit_position = 6378137.0; d.unit_velocity = 1000.0; d.unit_u = 1.0; d.unit_t = 597.0;
  d.dx = 1e-8; d.wind_rows = 3; d.wind_table = &wind[0][0]; d.ca_rows = 2; d.ca_table = &ca[0][0];
  d.device = GEL_DEVICE_NONE;
  gel_problem* p = NULL;
  REQUIRE(gel_problem_create(&d, &p) == GEL_OK && p);

  enum { B = 7, WA = 3, WB = 4 };
  double* a = calloc((size_t)B * 4 * WA, sizeof(double));   /* room for inc = 4 */
  double* b = calloc((size_t)B * WB, sizeof(double));
  double* C = malloc(sizeof(double) * WA * WB);
  double* sa = malloc(sizeof(double) * WA * 2);
  double* sb = malloc(sizeof(double) * WB * 2);
  double info[2];
  REQUIRE(a && b && C && sa && sb);
  const comom_fn forms[2] = {gel_batch_comoments, gel_batch_comoments_device};
  for (int f = 0; f < 2; f++) {
    const comom_fn call = forms[f];
    REQUIRE(call(NULL, B, WA, 1, WA, a, WB, 1, WB, b, C, sa, sb, info) == GEL_ERR_ARG);
    REQUIRE(call(p, -1, WA, 1, WA, a, WB, 1, WB, b, C, sa, sb, info) == GEL_ERR_ARG && strstr(gel_last_error(), "B < 0"));
    REQUIRE(call(p, B, -1, 1, WA, a, WB, 1, WB, b, C, sa, sb, info) == GEL_ERR_ARG && strstr(gel_last_error(), "W < 0"));
    REQUIRE(call(p, B, WA, 1, WA, a, -1, 1, WB, b, C, sa, sb, info) == GEL_ERR_ARG && strstr(gel_last_error(), "W < 0"));
    REQUIRE(call(p, B, WA, 0, WA, a, WB, 1, WB, b, C, sa, sb, info) == GEL_ERR_ARG && strstr(gel_last_error(), "inc < 1"));
    REQUIRE(call(p, B, WA, 1, WA, a, WB, -2, WB, b, C, sa, sb, info) == GEL_ERR_ARG && strstr(gel_last_error(), "inc < 1"));
    REQUIRE(call(p, B, WA, 1, WA - 1, a, WB, 1, WB, b, C, sa, sb, info) == GEL_ERR_ARG && strstr(gel_last_error(), "lda"));
    REQUIRE(call(p, B, WA, 4, 4 * (WA - 1), a, WB, 1, WB, b, C, sa, sb, info) == GEL_ERR_ARG && strstr(gel_last_error(), "lda"));
    REQUIRE(call(p, B, WA, 1, WA, a, WB, 1, WB - 1, b, C, sa, sb, info) == GEL_ERR_ARG && strstr(gel_last_error(), "ldb"));
    REQUIRE(call(p, B, WA, 1, WA, NULL, WB, 1, WB, b, C, sa, sb, info) == GEL_ERR_ARG && strstr(gel_last_error(), "a is NULL"));
    REQUIRE(call(p, B, WA, 1, WA, a, WB, 1, WB, b, NULL, sa, sb, info) == GEL_ERR_ARG && strstr(gel_last_error(), "C is NULL"));
    REQUIRE(call(p, B, WA, 1, WA, a, WB, 1, WB, b, C, sa, sb, NULL) == GEL_ERR_ARG && strstr(gel_last_error(), "info is NULL"));
    REQUIRE(call(p, B, WA, 1, WA, a, 0, 0, 0, NULL, C, sa, sb, info) == GEL_ERR_ARG && strstr(gel_last_error(), "self form"));
    /* valid calls reach the device check: no CPU fallback */
    REQUIRE(call(p, B, WA, 1, WA, a, WB, 1, WB, b, C, sa, sb, info) == GEL_ERR_HIP && strstr(gel_last_error(), "host-only"));
    REQUIRE(call(p, B, WA, 4, 4 * (WA - 1) + 1, a, WB, 1, WB, b, C, NULL, NULL, info) == GEL_ERR_HIP);
    REQUIRE(call(p, B, WA, 1, WA, a, 0, 0, 0, NULL, C, sa, NULL, info) == GEL_ERR_HIP);   /* the self form ignores Wb, incb, ldb */
    REQUIRE(call(p, 0, WA, 1, WA, NULL, WB, 1, WB, b, C, sa, sb, info) == GEL_ERR_HIP);
    REQUIRE(call(p, B, 0, 1, 0, NULL, WB, 1, WB, b, NULL, NULL, NULL, info) == GEL_ERR_HIP);
  }

  gel_comoments_info ci;
  REQUIRE(gel_batch_comoments_info(p, 65536, 24, 13260, 0, &ci) == GEL_OK);
  REQUIRE(ci.block == 256 && ci.tile_a >= 1 && ci.tile_b >= 1 && ci.slab_rows == 24);
  REQUIRE(ci.slab_cols >= 1 && ci.slabs * ci.slab_cols >= 13260 && ci.workspace_bytes <= ci.workspace_cap_bytes);
  REQUIRE(ci.workspace_cap_bytes == (int64_t)256 << 20 && ci.passes_a >= 2 && ci.passes_b == 2);
  REQUIRE(gel_batch_comoments_info(p, 300, 34, 0, 1, &ci) == GEL_OK && ci.slabs == 1 && ci.slab_cols == 34 && ci.passes_b == 0);
  REQUIRE(gel_batch_comoments_info(p, 0, 5, 5, 0, &ci) == GEL_OK && ci.passes_a == 0 && ci.slabs == 1);
  REQUIRE(gel_batch_comoments_info(p, 5, 0, 5, 0, &ci) == GEL_OK && ci.slabs == 0);
  REQUIRE(gel_batch_comoments_info(NULL, 5, 5, 5, 0, &ci) == GEL_ERR_ARG && gel_batch_comoments_info(p, 5, 5, 5, 0, NULL) == GEL_ERR_ARG);
  REQUIRE(gel_batch_comoments_info(p, -1, 5, 5, 0, &ci) == GEL_ERR_ARG && gel_batch_comoments_info(p, 5, -1, 5, 0, &ci) == GEL_ERR_ARG);
  REQUIRE(gel_batch_comoments_info(p, 5, 5, -1, 0, &ci) == GEL_ERR_ARG && gel_batch_comoments_info(p, 5, 5, -1, 1, &ci) == GEL_OK);

  free(a); free(b); free(C); free(sa); free(sb);
  REQUIRE(gel_problem_destroy(p) == GEL_OK);
  printf("COMOMENTS_SANITIZE_OK\n");
  return 0;
}
