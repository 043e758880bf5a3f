/* The tangent-linear propagation's entry points under AddressSanitizer + UBSan (CPU build only; nothing is launched): on plans of a
 * ragged host-only problem in all three modes, gel_prop_tangent_info against the plan's own workspace arithmetic and its refusals,
 * and every refusal of gel_propagate_tangent / gel_propagate_tangent_device, the host-only handle's among them -- each decided
 * before a buffer is looked at.  Prints FLIGHT_TANGENT_SANITIZE_OK on success. */
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
  const int32_t modes[3] = {0, GEL_PROP_RESTART_NODE, GEL_PROP_CHAIN};
  for (int m = 0; m < 3; m++) {
    gel_prop_plan* pl = NULL;
    REQUIRE(gel_prop_plan_create(p, steps, modes[m], &pl) == GEL_OK && pl);
    int64_t pi[6], ti[3];
    REQUIRE(gel_prop_plan_info(pl, pi) == GEL_OK);
    const int64_t set = pi[4], cap = (int64_t)1 << 30;
    const int32_t Ps[4] = {1, 5, 75, 4096};
    for (int i = 0; i < 4; i++) {
      for (int32_t shared = 0; shared < 2; shared++) {
        const int64_t P = Ps[i], B = 100000;
        REQUIRE(gel_prop_tangent_info(pl, (int32_t)B, (int32_t)P, shared, ti) == GEL_OK);
        const int64_t per_vec = shared ? set : set * (1 + P), fixed = shared ? set * ((P + 63) / 64 * 64) : 0;
        int64_t vs = (cap - fixed) / per_vec / 64 * 64;
        if (vs > (1 << 20)) vs = 1 << 20;
        if (vs > 0x7fffffff / P / 64 * 64) vs = 0x7fffffff / P / 64 * 64;
        if (vs < 64) vs = 64;
        REQUIRE(ti[0] == set && ti[1] == vs * P && ti[2] == (B + vs - 1) / vs);
        REQUIRE(ti[1] % (64 * P) == 0);
      }
    }
    REQUIRE(gel_prop_tangent_info(pl, 0, 1, 0, ti) == GEL_OK && ti[2] == 0);
    REQUIRE(gel_prop_tangent_info(pl, 1, 0, 0, ti) == GEL_ERR_ARG);
    REQUIRE(gel_prop_tangent_info(pl, -1, 1, 0, ti) == GEL_ERR_ARG);
    REQUIRE(gel_prop_tangent_info(pl, 1, 1, 2, ti) == GEL_ERR_ARG);
    REQUIRE(gel_prop_tangent_info(pl, 65536, 65536, 0, ti) == GEL_ERR_ARG);
    REQUIRE(gel_prop_tangent_info(NULL, 1, 1, 0, ti) == GEL_ERR_ARG && gel_prop_tangent_info(pl, 1, 1, 0, NULL) == GEL_ERR_ARG);
    /* the refusals, none of which reads a buffer: one double each is enough */
    double x[1] = {0.0}, y[1], dy[1], s1[1] = {1.0}, f[1] = {1.0};
    REQUIRE(gel_propagate_tangent(pl, 1, 0, 0, x, f, s1, s1, y, dy) == GEL_ERR_ARG);              /* P < 1 */
    REQUIRE(gel_propagate_tangent(pl, 65536, 65536, 1, x, f, s1, s1, y, dy) == GEL_ERR_ARG);      /* B P > 2^31 - 1 */
    REQUIRE(gel_propagate_tangent(pl, 1, 1, 0, x, f, NULL, NULL, y, dy) == GEL_ERR_ARG);          /* both seeds NULL */
    REQUIRE(gel_propagate_tangent(pl, 1, 1, 2, x, f, s1, s1, y, dy) == GEL_ERR_ARG);              /* shared not 0 / 1 */
    REQUIRE(gel_propagate_tangent(pl, 1, 1, -1, x, f, s1, s1, y, dy) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_tangent(pl, -1, 1, 0, x, f, s1, s1, y, dy) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_tangent(pl, 1, 1, 0, NULL, f, s1, s1, y, dy) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_tangent(pl, 1, 1, 0, x, f, s1, s1, y, NULL) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_tangent(NULL, 1, 1, 0, x, f, s1, s1, y, dy) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_tangent(pl, 1, 1, 0, x, f, s1, NULL, y, dy) == GEL_ERR_ARG);            /* a host-only handle */
    REQUIRE(strstr(gel_last_error(), "host-only") != NULL);
    REQUIRE(gel_propagate_tangent(pl, 1, 1, 1, x, NULL, NULL, s1, y, dy) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_tangent_device(pl, 1, 0, 0, x, f, s1, s1, y, dy) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_tangent_device(pl, 1, 1, 0, x, f, NULL, NULL, y, dy) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_tangent_device(pl, 1, 1, 3, x, f, s1, s1, y, dy) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_tangent_device(pl, 65536, 65536, 0, x, f, s1, s1, y, dy) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_tangent_device(pl, 1, 1, 0, x, f, s1, s1, y, dy) == GEL_ERR_ARG);       /* a host-only handle */
    REQUIRE(strstr(gel_last_error(), "host-only") != NULL);
    REQUIRE(gel_prop_plan_destroy(pl) == GEL_OK);
  }
  REQUIRE(gel_problem_destroy(p) == GEL_OK);
  printf("FLIGHT_TANGENT_SANITIZE_OK\n");
  return 0;
}
