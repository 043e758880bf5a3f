/* The propagation plan's builder under AddressSanitizer + UBSan (CPU build only; nothing is launched): section, node and chain
 * plans of a ragged host-only problem, gel_prop_plan_info in each mode, gel_prop_matrices into exactly sized heap buffers, the
 * refusals (both mode flags, an unknown flag, the per-section cap, the chain's cap on the SUM of steps n at 2^20 and one below),
 * and the evaluation calls' refusal of a host-only handle.  Prints FLIGHT_SANITIZE_OK on success. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/gelato_amd.h"

#define REQUIRE(c)                                                          \
  do {                                                                      \
    if (!(c)) { fprintf(stderr, "REQUIRE failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, gel_last_error()); return 1; } \
  } while (0)

int main(void) {
  enum { S = 5 };
  const int32_t nn[S] = {2, 3, 4, 17, 4};
  const double thrust[S] = {420000.0, 0.0, 420000.0, 30700.0, 0.0};
  const double mdot[S] = {140.0, 0.0, 140.0, 9.8, 0.0};
  const double area[S] = {2.21, 2.21, 2.21, 0.0, 0.0};
  const double nozzle[S] = {0.68, 0.0, 0.68, 0.0, 0.0};
  const int32_t on[S] = {1, 0, 1, 1, 0};
  const int32_t hold[S] = {1, 0, 0, 1, 0};
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

  const int32_t steps[S] = {1, 3, 2, 1, 5};
  int64_t sum = 0, mx = 0, mk = 0, pts = 0, sampled = 0;
  for (int s = 0; s < S; s++) {
    const int64_t kn = (int64_t)steps[s] * nn[s];
    sum += kn;
    if (kn > mx) mx = kn;
    if (steps[s] > mk) mk = steps[s];
    pts += 2 * kn + 1;
    if (!hold[s]) sampled += 2 * kn + 1;
  }
  const int32_t modes[3] = {0, GEL_PROP_RESTART_NODE, GEL_PROP_CHAIN};
  const int64_t lane[3] = {mx, mk, sum};
  for (int m = 0; m < 3; m++) {
    gel_prop_plan* pl = NULL;
    REQUIRE(gel_prop_plan_create(p, steps, modes[m], &pl) == GEL_OK && pl);
    int64_t info[6];
    REQUIRE(gel_prop_plan_info(pl, info) == GEL_OK);
    REQUIRE(info[0] == S && info[1] == modes[m] && info[2] == pts && info[3] == lane[m] && info[4] == 16 * sampled);
    REQUIRE(info[5] >= 64 && info[5] % 64 == 0);
    for (int s = 0; s < S; s++) {
      const size_t Pp = 2 * (size_t)steps[s] * nn[s] + 1;
      double* z = malloc(sizeof(double) * Pp);
      double* Wu = malloc(sizeof(double) * Pp * nn[s]);
      int32_t* cu = malloc(sizeof(int32_t) * Pp);
      REQUIRE(gel_prop_matrices(pl, s, z, Wu, cu) == GEL_OK);
      REQUIRE(z[0] == -1.0 && z[Pp - 1] == 1.0 && cu[0] == -1 && cu[Pp - 1] == nn[s] - 1);
      for (size_t l = 1; l < Pp; l++) REQUIRE(z[l] > z[l - 1]);
      REQUIRE(gel_prop_matrices(pl, s, NULL, NULL, NULL) == GEL_OK);
      free(z); free(Wu); free(cu);
    }
    REQUIRE(gel_prop_matrices(pl, S, NULL, NULL, NULL) != GEL_OK && gel_prop_matrices(pl, -1, NULL, NULL, NULL) != GEL_OK);
    /* a host-only handle never evaluates (no CPU fallback); B = 0 and bad arguments are judged first */
    double x[1] = {0.0}, y[1], f[1] = {1.0};
    REQUIRE(gel_propagate(pl, 1, x, y, NULL) == GEL_ERR_HIP);
    REQUIRE(gel_propagate_dispersed(pl, 1, x, f, y, NULL) == GEL_ERR_HIP);
    REQUIRE(gel_propagate_device(pl, 1, x, y, NULL) == GEL_ERR_HIP);
    REQUIRE(gel_propagate_dispersed_device(pl, 1, x, f, y, NULL) == GEL_ERR_HIP);
    REQUIRE(gel_propagate_dispersed(pl, -1, x, f, y, NULL) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_dispersed(pl, 1, NULL, f, y, NULL) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_dispersed_device(NULL, 1, x, f, y, NULL) == GEL_ERR_ARG);
    REQUIRE(gel_prop_plan_destroy(pl) == GEL_OK);
  }
  /* refusals */
  gel_prop_plan* q = NULL;
  REQUIRE(gel_prop_plan_create(p, steps, GEL_PROP_CHAIN | GEL_PROP_RESTART_NODE, &q) == GEL_ERR_ARG && q == NULL);
  REQUIRE(strstr(gel_last_error(), "exclude"));
  REQUIRE(gel_prop_plan_create(p, steps, 4, &q) == GEL_ERR_ARG && q == NULL);
  REQUIRE(gel_prop_plan_create(p, NULL, GEL_PROP_CHAIN, &q) == GEL_ERR_ARG);
  int32_t big[S] = {1, 1, 1, 1, 1};
  big[1] = 0;
  REQUIRE(gel_prop_plan_create(p, big, GEL_PROP_CHAIN, &q) == GEL_ERR_ARG && q == NULL);
  /* the chain's cap: sum steps n = 2 a + 3 b + 4 c + 17 e + 4 f.  With a = c = e = f = 1 the rest is 27, and 2^20 - 28 is a multiple
   * of 3 (2^20 = 1 mod 3): b = (2^20 - 28) / 3 gives 2^20 - 1, which is accepted; a = 2 then gives 2^20 + 1, which is refused */
  big[0] = 1; big[2] = 1; big[3] = 1; big[4] = 1;
  big[1] = ((1 << 20) - 27 - 1) / 3;
  REQUIRE(2 * big[0] + 3 * big[1] + 4 * big[2] + 17 * big[3] + 4 * big[4] == (1 << 20) - 1);
  REQUIRE(gel_prop_plan_create(p, big, GEL_PROP_CHAIN, &q) == GEL_OK && q);
  REQUIRE(gel_prop_plan_destroy(q) == GEL_OK);
  q = NULL;
  big[0] = 2;                                                     /* 2^20 + 1 */
  REQUIRE(gel_prop_plan_create(p, big, 0, &q) == GEL_OK && q);   /* section mode: every phase is below the cap on its own */
  REQUIRE(gel_prop_plan_destroy(q) == GEL_OK);
  q = NULL;
  REQUIRE(gel_prop_plan_create(p, big, GEL_PROP_CHAIN, &q) == GEL_ERR_ARG && q == NULL && strstr(gel_last_error(), "sum"));
  big[0] = 1; big[1] = (1 << 20) / 3 + 1;                         /* one phase alone above 2^20: refused in every mode */
  for (int m = 0; m < 3; m++) REQUIRE(gel_prop_plan_create(p, big, modes[m], &q) == GEL_ERR_ARG && q == NULL);
  REQUIRE(gel_prop_plan_destroy(NULL) == GEL_OK);
  REQUIRE(gel_problem_destroy(p) == GEL_OK);
  printf("FLIGHT_SANITIZE_OK\n");
  return 0;
}
