/* The tangent and the adjoint flight under a wind ensemble, host side, under AddressSanitizer + UBSan (CPU build
 * only; nothing is launched): on plans of a ragged host-only problem, with ensembles created and assigned on it and on a second
 * handle, every refusal of the four gel_propagate_{tangent,adjoint}_ensemble[_device] calls -- the parent's rules, then the
 * ensemble's, then the host-only handle -- each decided before a buffer is looked at: every buffer passed is ONE double.
 * ens == NULL is the parent call.  Prints ENSEMBLE_TANGENT_SANITIZE_OK on success. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/gelato_amd.h"

#define REQUIRE(c)                                                          \
  do {                                                                      \
    if (!(c)) { fprintf(stderr, "REQUIRE failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, gel_last_error()); return 1; } \
  } while (0)
#define REFUSED(call, text) REQUIRE((call) == GEL_ERR_ARG && strstr(gel_last_error(), text) != NULL)

int main(void) {
  enum { S = 5, B = 4 };
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
  gel_problem *p = NULL, *other = NULL;
  REQUIRE(gel_problem_create(&d, &p) == GEL_OK && p);
  REQUIRE(gel_problem_create(&d, &other) == GEL_OK && other);

  /* two members of four rows */
  const double tables[2][4][3] = {{{0.0, 1.0, 2.0}, {3000.0, 4.0, -2.0}, {9000.0, 12.0, 1.0}, {30000.0, 0.0, 0.0}},
                                  {{100.0, -1.0, 0.5}, {2500.0, 6.0, 3.0}, {11000.0, -8.0, 7.0}, {25000.0, 2.0, 2.0}}};
  const int32_t m4[B] = {0, -1, 1, 1};
  gel_wind_ensemble *ens = NULL, *shrt = NULL, *foreign = NULL, *unassigned = NULL, *empty = NULL;
  REQUIRE(gel_wind_ensemble_create(p, 2, 4, &tables[0][0][0], &ens) == GEL_OK && gel_wind_ensemble_assign(ens, B, m4) == GEL_OK);
  REQUIRE(gel_wind_ensemble_create(p, 2, 4, &tables[0][0][0], &shrt) == GEL_OK && gel_wind_ensemble_assign(shrt, B - 1, m4) == GEL_OK);
  REQUIRE(gel_wind_ensemble_create(other, 2, 4, &tables[0][0][0], &foreign) == GEL_OK && gel_wind_ensemble_assign(foreign, B, m4) == GEL_OK);
  REQUIRE(gel_wind_ensemble_create(p, 2, 4, &tables[0][0][0], &unassigned) == GEL_OK);
  REQUIRE(gel_wind_ensemble_create(p, 2, 4, &tables[0][0][0], &empty) == GEL_OK && gel_wind_ensemble_assign(empty, 0, NULL) == GEL_OK);

  const int32_t steps[S] = {1, 3, 2, 1, 5};
  const int32_t modes[3] = {0, GEL_PROP_CHAIN, GEL_PROP_RESTART_NODE};
  double x[1] = {0.0}, y[1], dy[1], gx[1], gd[1], lam[1] = {1.0}, f[1] = {1.0}, dx[1] = {1.0}, df[1] = {1.0};
  for (int m = 0; m < 3; m++) {
    gel_prop_plan* pl = NULL;
    REQUIRE(gel_prop_plan_create(p, steps, modes[m], &pl) == GEL_OK && pl);
    int64_t before[3], after[3];
    REQUIRE(gel_prop_tangent_info(pl, B, 3, 1, before) == GEL_OK);
    /* ---- the tangent: all three plan modes ---- */
    REFUSED(gel_propagate_tangent_ensemble(pl, B, 3, 1, x, f, dx, df, ens, y, dy), "host-only");
    REFUSED(gel_propagate_tangent_ensemble_device(pl, B, 3, 1, x, f, dx, df, ens, y, dy), "host-only");
    REFUSED(gel_propagate_tangent_ensemble(pl, B, 3, 1, x, f, dx, df, NULL, y, dy), "host-only");            /* the parent call */
    REFUSED(gel_propagate_tangent_ensemble(pl, B, 3, 0, x, f, dx, df, shrt, y, dy), "assigned 3 vectors, the call has B = 4");
    REFUSED(gel_propagate_tangent_ensemble_device(pl, B, 3, 0, x, f, dx, df, shrt, y, dy), "assigned 3 vectors, the call has B = 4");
    REFUSED(gel_propagate_tangent_ensemble(pl, B, 3, 0, x, f, dx, df, foreign, y, dy), "another handle");
    REFUSED(gel_propagate_tangent_ensemble_device(pl, B, 3, 0, x, f, dx, df, foreign, y, dy), "another handle");
    REFUSED(gel_propagate_tangent_ensemble(pl, B, 3, 0, x, f, dx, df, unassigned, y, dy), "no vectors yet");
    REFUSED(gel_propagate_tangent_ensemble(pl, B, 0, 1, x, f, dx, df, shrt, y, dy), "P < 1");                /* the parent's rules first */
    REFUSED(gel_propagate_tangent_ensemble_device(pl, B, 3, 1, x, f, NULL, NULL, shrt, y, dy), "both seeds");
    REFUSED(gel_propagate_tangent_ensemble(pl, B, 3, 2, x, f, dx, df, shrt, y, dy), "shared is neither");
    REFUSED(gel_propagate_tangent_ensemble(pl, -1, 3, 1, x, f, dx, df, shrt, y, dy), "B < 0");
    REFUSED(gel_propagate_tangent_ensemble(pl, 65536, 65536, 1, x, f, dx, df, ens, y, dy), "2^31");
    REFUSED(gel_propagate_tangent_ensemble(NULL, B, 3, 1, x, f, dx, df, ens, y, dy), "null plan");
    REFUSED(gel_propagate_tangent_ensemble(pl, 0, 3, 1, NULL, NULL, dx, NULL, empty, NULL, NULL), "host-only");   /* even with B = 0 */
    REFUSED(gel_propagate_tangent_ensemble(pl, 0, 3, 1, NULL, NULL, dx, NULL, ens, NULL, NULL), "assigned 4 vectors, the call has B = 0");
    REQUIRE(gel_prop_tangent_info(pl, B, 3, 1, after) == GEL_OK && memcmp(before, after, sizeof before) == 0);
    /* ---- the adjoint ---- */
    if (modes[m] == GEL_PROP_RESTART_NODE) {
      REFUSED(gel_propagate_adjoint_ensemble(pl, B, 2, 1, x, f, lam, ens, y, gx, gd), "GEL_PROP_RESTART_NODE");
      REFUSED(gel_propagate_adjoint_ensemble_device(pl, B, 2, 1, x, f, lam, shrt, y, gx, gd), "GEL_PROP_RESTART_NODE");
      REFUSED(gel_propagate_adjoint_ensemble(pl, B, 2, 1, x, f, lam, NULL, y, gx, gd), "GEL_PROP_RESTART_NODE");
      REQUIRE(gel_prop_plan_destroy(pl) == GEL_OK);
      continue;
    }
    REQUIRE(gel_prop_adjoint_info(pl, B, 2, 1, before) == GEL_OK);
    REFUSED(gel_propagate_adjoint_ensemble(pl, B, 2, 1, x, f, lam, ens, y, gx, gd), "host-only");
    REFUSED(gel_propagate_adjoint_ensemble_device(pl, B, 2, 1, x, f, lam, ens, y, gx, NULL), "host-only");
    REFUSED(gel_propagate_adjoint_ensemble(pl, B, 2, 1, x, f, lam, NULL, y, gx, gd), "host-only");             /* the parent call */
    REFUSED(gel_propagate_adjoint_ensemble(pl, B, 2, 0, x, f, lam, shrt, y, gx, gd), "assigned 3 vectors, the call has B = 4");
    REFUSED(gel_propagate_adjoint_ensemble_device(pl, B, 2, 0, x, f, lam, shrt, y, gx, gd), "assigned 3 vectors, the call has B = 4");
    REFUSED(gel_propagate_adjoint_ensemble(pl, B, 2, 0, x, f, lam, foreign, y, gx, gd), "another handle");
    REFUSED(gel_propagate_adjoint_ensemble_device(pl, B, 2, 0, x, f, lam, foreign, y, gx, gd), "another handle");
    REFUSED(gel_propagate_adjoint_ensemble(pl, B, 2, 0, x, f, lam, unassigned, y, gx, gd), "no vectors yet");
    REFUSED(gel_propagate_adjoint_ensemble(pl, B, 0, 1, x, f, lam, shrt, y, gx, gd), "Q < 1");                 /* the parent's rules first */
    REFUSED(gel_propagate_adjoint_ensemble_device(pl, B, 2, 1, x, f, NULL, shrt, y, gx, gd), "lam is NULL");
    REFUSED(gel_propagate_adjoint_ensemble(pl, B, 2, 3, x, f, lam, shrt, y, gx, gd), "shared is neither");
    REFUSED(gel_propagate_adjoint_ensemble(pl, B, 1 << 24, 0, x, f, lam, shrt, y, gx, gd), "1 GB");
    REFUSED(gel_propagate_adjoint_ensemble(NULL, B, 2, 1, x, f, lam, ens, y, gx, gd), "null plan");
    REFUSED(gel_propagate_adjoint_ensemble(pl, 0, 2, 1, NULL, NULL, lam, empty, NULL, NULL, NULL), "host-only");  /* even with B = 0 */
    REQUIRE(gel_prop_adjoint_info(pl, B, 2, 1, after) == GEL_OK && memcmp(before, after, sizeof before) == 0);
    REQUIRE(gel_prop_plan_destroy(pl) == GEL_OK);
  }
  REQUIRE(gel_wind_ensemble_destroy(ens) == GEL_OK && gel_wind_ensemble_destroy(shrt) == GEL_OK && gel_wind_ensemble_destroy(foreign) == GEL_OK);
  REQUIRE(gel_wind_ensemble_destroy(unassigned) == GEL_OK && gel_wind_ensemble_destroy(empty) == GEL_OK);
  REQUIRE(gel_problem_destroy(other) == GEL_OK && gel_problem_destroy(p) == GEL_OK);
  printf("ENSEMBLE_TANGENT_SANITIZE_OK\n");
  return 0;
}
