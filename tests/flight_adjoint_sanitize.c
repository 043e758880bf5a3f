/* The adjoint flight's entry points under AddressSanitizer + UBSan (CPU build only; nothing is launched): on plans of a ragged
 * host-only problem, gel_prop_adjoint_info against the plan's own workspace arithmetic and its refusals, and every refusal of
 * gel_propagate_adjoint / gel_propagate_adjoint_device, the host-only handle's and the node-restart plan's among them -- each decided
 * before a buffer is looked at.  Prints FLIGHT_ADJOINT_SANITIZE_OK on success. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/gelato_amd.h"

#define REQUIRE(c)                                                          \
  do {                                                                      \
    if (!(c)) { fprintf(stderr, "REQUIRE failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, gel_last_error()); return 1; } \
  } while (0)

int main(void) {
  enum { S = 5, N = 30 };
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
  const int32_t modes[3] = {0, GEL_PROP_CHAIN, GEL_PROP_RESTART_NODE};
  double x[1] = {0.0}, y[1], gx[1], gd[1], lam[1] = {1.0}, f[1] = {1.0};
  for (int m = 0; m < 3; m++) {
    gel_prop_plan* pl = NULL;
    REQUIRE(gel_prop_plan_create(p, steps, modes[m], &pl) == GEL_OK && pl);
    int64_t pi[6], ai[3];
    REQUIRE(gel_prop_plan_info(pl, pi) == GEL_OK);
    if (modes[m] == GEL_PROP_RESTART_NODE) {
      REQUIRE(gel_prop_adjoint_info(pl, 1, 1, 0, ai) == GEL_ERR_ARG && strstr(gel_last_error(), "GEL_PROP_RESTART_NODE") != NULL);
      REQUIRE(gel_propagate_adjoint(pl, 1, 1, 0, x, f, lam, y, gx, gd) == GEL_ERR_ARG && strstr(gel_last_error(), "GEL_PROP_RESTART_NODE") != NULL);
      REQUIRE(gel_propagate_adjoint_device(pl, 1, 1, 0, x, f, lam, y, gx, gd) == GEL_ERR_ARG);
      REQUIRE(gel_prop_plan_destroy(pl) == GEL_OK);
      continue;
    }
    const int64_t set = pi[4], lane = set + 8 * S + 88 * (5 - 1) /* the largest steps[s] */, cap = (int64_t)1 << 30;
    const int32_t Qs[4] = {1, 7, 75, 4096};
    for (int i = 0; i < 4; i++) {
      for (int32_t shared = 0; shared < 2; shared++) {
        const int64_t Q = Qs[i], B = 100000;
        REQUIRE(gel_prop_adjoint_info(pl, (int32_t)B, (int32_t)Q, shared, ai) == GEL_OK);
        int64_t vs = cap / (set + Q * lane) / 64 * 64;
        if (vs > (1 << 20)) vs = 1 << 20;
        int64_t lanes = (int64_t)0x7fffffff / (N + 1) * 256;
        if (lanes > 0x7fffffff) lanes = 0x7fffffff;
        if (vs > lanes / Q / 64 * 64) vs = lanes / Q / 64 * 64;
        REQUIRE(vs >= 64 && ai[0] == lane && ai[1] == vs * Q && ai[2] == (B + vs - 1) / vs);
      }
    }
    REQUIRE(gel_prop_adjoint_info(pl, 0, 1, 0, ai) == GEL_OK && ai[2] == 0);
    REQUIRE(gel_prop_adjoint_info(pl, 1, 0, 0, ai) == GEL_ERR_ARG);
    REQUIRE(gel_prop_adjoint_info(pl, -1, 1, 0, ai) == GEL_ERR_ARG);
    REQUIRE(gel_prop_adjoint_info(pl, 1, 1, 2, ai) == GEL_ERR_ARG);
    REQUIRE(gel_prop_adjoint_info(pl, 65536, 65536, 0, ai) == GEL_ERR_ARG);
    REQUIRE(gel_prop_adjoint_info(pl, 1, 1 << 24, 0, ai) == GEL_ERR_ARG && strstr(gel_last_error(), "1 GB") != NULL);
    REQUIRE(gel_prop_adjoint_info(NULL, 1, 1, 0, ai) == GEL_ERR_ARG && gel_prop_adjoint_info(pl, 1, 1, 0, NULL) == GEL_ERR_ARG);
    /* the refusals, none of which reads a buffer: one double each is enough */
    REQUIRE(gel_propagate_adjoint(pl, 1, 0, 0, x, f, lam, y, gx, gd) == GEL_ERR_ARG);              /* Q < 1 */
    REQUIRE(gel_propagate_adjoint(pl, 65536, 65536, 1, x, f, lam, y, gx, gd) == GEL_ERR_ARG);      /* B Q > 2^31 - 1 */
    REQUIRE(gel_propagate_adjoint(pl, 1, 1, 0, x, f, NULL, y, gx, gd) == GEL_ERR_ARG);             /* lam NULL */
    REQUIRE(strstr(gel_last_error(), "lam is NULL") != NULL);
    REQUIRE(gel_propagate_adjoint(pl, 1, 1, 2, x, f, lam, y, gx, gd) == GEL_ERR_ARG);              /* shared not 0 / 1 */
    REQUIRE(gel_propagate_adjoint(pl, 1, 1, -1, x, f, lam, y, gx, gd) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_adjoint(pl, -1, 1, 0, x, f, lam, y, gx, gd) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_adjoint(pl, 1, 1 << 24, 0, x, f, lam, y, gx, gd) == GEL_ERR_ARG);        /* the workspace */
    REQUIRE(gel_propagate_adjoint(NULL, 1, 1, 0, x, f, lam, y, gx, gd) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_adjoint(pl, 1, 1, 0, x, f, lam, y, gx, NULL) == GEL_ERR_ARG);            /* a host-only handle */
    REQUIRE(strstr(gel_last_error(), "host-only") != NULL);
    REQUIRE(gel_propagate_adjoint(pl, 0, 1, 1, NULL, NULL, lam, NULL, NULL, NULL) == GEL_ERR_ARG); /* even with B = 0 */
    REQUIRE(gel_propagate_adjoint_device(pl, 1, 0, 0, x, f, lam, y, gx, gd) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_adjoint_device(pl, 1, 1, 0, x, f, NULL, y, gx, gd) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_adjoint_device(pl, 1, 1, 3, x, f, lam, y, gx, gd) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_adjoint_device(pl, 65536, 65536, 0, x, f, lam, y, gx, gd) == GEL_ERR_ARG);
    REQUIRE(gel_propagate_adjoint_device(pl, 1, 1, 0, x, f, lam, y, gx, gd) == GEL_ERR_ARG);       /* a host-only handle */
    REQUIRE(strstr(gel_last_error(), "host-only") != NULL);
    REQUIRE(gel_prop_plan_destroy(pl) == GEL_OK);
  }
  REQUIRE(gel_problem_destroy(p) == GEL_OK);
  printf("FLIGHT_ADJOINT_SANITIZE_OK\n");
  return 0;
}
