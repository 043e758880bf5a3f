/* The wind-profile sensitivities of the flight, host side, under AddressSanitizer + UBSan (CPU build only; nothing is
 * launched): on plans of a ragged host-only problem, with ensembles created and assigned on it and on a second handle, every refusal
 * of gel_propagate_{tangent,adjoint}_wind[_device] -- the parents' rules, then the ensemble's, then the host-only handle -- each
 * decided before a buffer is looked at: every buffer passed is ONE double.  dwind == NULL / gwind == NULL are the parents' calls.
 * gel_prop_wind_rows and gel_prop_adjoint_wind_info answer on host-only handles.  Prints FLIGHT_WIND_SANITIZE_OK on success. */
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

  /* two members of four rows; one of two rows (fewer than the handle's three) */
  const double tables[2][4][3] = {{{0.0, 1.0, 2.0}, {3000.0, 4.0, -2.0}, {9000.0, 12.0, 1.0}, {30000.0, 0.0, 0.0}},
                                  {{100.0, -1.0, 0.5}, {2500.0, 6.0, 3.0}, {11000.0, -8.0, 7.0}, {25000.0, 2.0, 2.0}}};
  const double two[2][3] = {{0.0, 1.0, 2.0}, {9000.0, 4.0, -2.0}};
  const int32_t m4[B] = {0, -1, 1, 1}, m0[B] = {0, 0, -1, 0};
  gel_wind_ensemble *ens = NULL, *shrt = NULL, *foreign = NULL, *unassigned = NULL, *small = NULL;
  REQUIRE(gel_wind_ensemble_create(p, 2, 4, &tables[0][0][0], &ens) == GEL_OK && gel_wind_ensemble_assign(ens, B, m4) == GEL_OK);
  REQUIRE(gel_wind_ensemble_create(p, 2, 4, &tables[0][0][0], &shrt) == GEL_OK && gel_wind_ensemble_assign(shrt, B - 1, m4) == GEL_OK);
  REQUIRE(gel_wind_ensemble_create(other, 2, 4, &tables[0][0][0], &foreign) == GEL_OK && gel_wind_ensemble_assign(foreign, B, m4) == GEL_OK);
  REQUIRE(gel_wind_ensemble_create(p, 2, 4, &tables[0][0][0], &unassigned) == GEL_OK);
  REQUIRE(gel_wind_ensemble_create(p, 1, 2, &two[0][0], &small) == GEL_OK && gel_wind_ensemble_assign(small, B, m0) == GEL_OK);

  const int32_t steps[S] = {1, 3, 2, 1, 5};
  const int32_t modes[3] = {0, GEL_PROP_CHAIN, GEL_PROP_RESTART_NODE};
  double x[1] = {0.0}, y[1], dy[1], gx[1], gd[1], gw[1], lam[1] = {1.0}, f[1] = {1.0}, dx[1] = {1.0}, df[1] = {1.0}, dw[1] = {1.0};
  for (int m = 0; m < 3; m++) {
    gel_prop_plan* pl = NULL;
    REQUIRE(gel_prop_plan_create(p, steps, modes[m], &pl) == GEL_OK && pl);
    /* ---- the row count ---- */
    int32_t Kg = -1;
    REQUIRE(gel_prop_wind_rows(pl, NULL, &Kg) == GEL_OK && Kg == 3);
    REQUIRE(gel_prop_wind_rows(pl, ens, &Kg) == GEL_OK && Kg == 4);
    REQUIRE(gel_prop_wind_rows(pl, unassigned, &Kg) == GEL_OK && Kg == 4);
    REQUIRE(gel_prop_wind_rows(pl, small, &Kg) == GEL_OK && Kg == 3);          /* the larger of the two */
    REFUSED(gel_prop_wind_rows(NULL, ens, &Kg), "gel_prop_wind_rows: null plan");
    REFUSED(gel_prop_wind_rows(pl, ens, NULL), "gel_prop_wind_rows: Kg is NULL");
    REFUSED(gel_prop_wind_rows(pl, foreign, &Kg), "gel_prop_wind_rows: the wind ensemble belongs to another handle");
    /* ---- the tangent: all three plan modes, every subset of the seeds ---- */
    REFUSED(gel_propagate_tangent_wind(pl, B, 3, 1, x, f, dx, df, dw, ens, y, dy), "gel_propagate_tangent_wind: the plan's handle is host-only");
    REFUSED(gel_propagate_tangent_wind_device(pl, B, 3, 1, x, f, dx, df, dw, ens, y, dy), "gel_propagate_tangent_wind_device: the plan's handle is host-only");
    REFUSED(gel_propagate_tangent_wind(pl, B, 3, 1, x, f, NULL, NULL, dw, NULL, y, dy), "host-only");          /* the wind seed alone */
    REFUSED(gel_propagate_tangent_wind(pl, B, 3, 0, x, NULL, dx, NULL, dw, NULL, y, dy), "host-only");
    REFUSED(gel_propagate_tangent_wind(pl, B, 3, 0, x, f, dx, df, NULL, ens, y, dy), "host-only");             /* the parent call */
    REFUSED(gel_propagate_tangent_wind_device(pl, B, 3, 1, x, f, NULL, NULL, NULL, shrt, y, dy), "all three seeds");
    REFUSED(gel_propagate_tangent_wind(pl, B, 3, 1, x, f, NULL, NULL, NULL, NULL, y, dy), "gel_propagate_tangent_wind: all three seeds");
    REFUSED(gel_propagate_tangent_wind(pl, B, 3, 0, x, f, dx, df, dw, shrt, y, dy), "assigned 3 vectors, the call has B = 4");
    REFUSED(gel_propagate_tangent_wind_device(pl, B, 3, 0, x, f, NULL, NULL, dw, shrt, y, dy), "assigned 3 vectors, the call has B = 4");
    REFUSED(gel_propagate_tangent_wind(pl, B, 3, 0, x, f, dx, df, dw, foreign, y, dy), "another handle");
    REFUSED(gel_propagate_tangent_wind(pl, B, 3, 0, x, f, dx, df, dw, unassigned, y, dy), "no vectors yet");
    REFUSED(gel_propagate_tangent_wind(pl, B, 0, 1, x, f, dx, df, dw, shrt, y, dy), "P < 1");                 /* the parent's rules first */
    REFUSED(gel_propagate_tangent_wind(pl, B, 3, 2, x, f, dx, df, dw, shrt, y, dy), "shared is neither");
    REFUSED(gel_propagate_tangent_wind(pl, -1, 3, 1, x, f, dx, df, dw, shrt, y, dy), "B < 0");
    REFUSED(gel_propagate_tangent_wind(pl, 65536, 65536, 1, x, f, dx, df, dw, ens, y, dy), "2^31");
    REFUSED(gel_propagate_tangent_wind(NULL, B, 3, 1, x, f, dx, df, dw, ens, y, dy), "gel_propagate_tangent_wind: null plan");
    REFUSED(gel_propagate_tangent_wind(pl, B, 3, 1, NULL, f, NULL, NULL, dw, ens, y, dy), "x, y or dy is NULL");
    /* ---- the adjoint ---- */
    int64_t info3[3], info[4], infow[4];
    if (modes[m] == GEL_PROP_RESTART_NODE) {
      REFUSED(gel_propagate_adjoint_wind(pl, B, 2, 1, x, f, lam, ens, y, gx, gd, gw), "GEL_PROP_RESTART_NODE");
      REFUSED(gel_propagate_adjoint_wind_device(pl, B, 2, 1, x, f, lam, shrt, y, gx, gd, gw), "GEL_PROP_RESTART_NODE");
      REFUSED(gel_propagate_adjoint_wind(pl, B, 2, 1, x, f, lam, NULL, y, gx, gd, NULL), "GEL_PROP_RESTART_NODE");
      REFUSED(gel_prop_adjoint_wind_info(pl, ens, B, 2, 1, 1, info), "gel_prop_adjoint_wind_info: a GEL_PROP_RESTART_NODE plan");
      REQUIRE(gel_prop_plan_destroy(pl) == GEL_OK);
      continue;
    }
    REFUSED(gel_propagate_adjoint_wind(pl, B, 2, 1, x, f, lam, ens, y, gx, gd, gw), "gel_propagate_adjoint_wind: the plan's handle is host-only");
    REFUSED(gel_propagate_adjoint_wind_device(pl, B, 2, 1, x, f, lam, ens, y, gx, NULL, gw), "gel_propagate_adjoint_wind_device: the plan's handle is host-only");
    REFUSED(gel_propagate_adjoint_wind(pl, B, 2, 1, x, f, lam, NULL, y, gx, gd, gw), "host-only");
    REFUSED(gel_propagate_adjoint_wind(pl, B, 2, 1, x, f, lam, ens, y, gx, gd, NULL), "host-only");            /* the parent call */
    REFUSED(gel_propagate_adjoint_wind(pl, B, 2, 0, x, f, lam, shrt, y, gx, gd, gw), "assigned 3 vectors, the call has B = 4");
    REFUSED(gel_propagate_adjoint_wind_device(pl, B, 2, 0, x, f, lam, shrt, y, gx, gd, gw), "assigned 3 vectors, the call has B = 4");
    REFUSED(gel_propagate_adjoint_wind(pl, B, 2, 0, x, f, lam, foreign, y, gx, gd, gw), "another handle");
    REFUSED(gel_propagate_adjoint_wind(pl, B, 2, 0, x, f, lam, unassigned, y, gx, gd, gw), "no vectors yet");
    REFUSED(gel_propagate_adjoint_wind(pl, B, 0, 1, x, f, lam, shrt, y, gx, gd, gw), "Q < 1");                /* the parent's rules first */
    REFUSED(gel_propagate_adjoint_wind_device(pl, B, 2, 1, x, f, NULL, shrt, y, gx, gd, gw), "lam is NULL");
    REFUSED(gel_propagate_adjoint_wind(pl, B, 2, 3, x, f, lam, shrt, y, gx, gd, gw), "shared is neither");
    REFUSED(gel_propagate_adjoint_wind(pl, B, 1 << 24, 0, x, f, lam, shrt, y, gx, gd, gw), "1 GB");
    REFUSED(gel_propagate_adjoint_wind(NULL, B, 2, 1, x, f, lam, ens, y, gx, gd, gw), "gel_propagate_adjoint_wind: null plan");
    REFUSED(gel_propagate_adjoint_wind(pl, 0, 2, 1, NULL, NULL, lam, NULL, NULL, NULL, NULL, gw), "host-only");  /* even with B = 0 */
    /* ---- the workspace figures: the parent's where gwind is not wanted, 16 Kg bytes per lane more where it is ---- */
    REQUIRE(gel_prop_adjoint_info(pl, B, 2, 1, info3) == GEL_OK);
    REQUIRE(gel_prop_adjoint_wind_info(pl, ens, B, 2, 1, 0, info) == GEL_OK && memcmp(info3, info, sizeof info3) == 0 && info[3] == 4);
    REQUIRE(gel_prop_adjoint_wind_info(pl, ens, B, 2, 1, 1, infow) == GEL_OK && infow[0] == info[0] + 16 * 4 && infow[3] == 4);
    REQUIRE(gel_prop_adjoint_wind_info(pl, NULL, B, 2, 0, 1, infow) == GEL_OK && infow[0] == info[0] + 16 * 3 && infow[3] == 3);
    REQUIRE(infow[1] % (64 * 2) == 0 && infow[1] <= info[1] && infow[2] >= 1);
    REFUSED(gel_prop_adjoint_wind_info(pl, ens, B, 2, 1, 1, NULL), "gel_prop_adjoint_wind_info: info is NULL");
    REFUSED(gel_prop_adjoint_wind_info(NULL, ens, B, 2, 1, 1, info), "gel_prop_adjoint_wind_info: null plan");
    REFUSED(gel_prop_adjoint_wind_info(pl, foreign, B, 2, 1, 1, info), "gel_prop_adjoint_wind_info: the wind ensemble belongs to another handle");
    REFUSED(gel_prop_adjoint_wind_info(pl, ens, B, 0, 1, 1, info), "Q < 1");
    REFUSED(gel_prop_adjoint_wind_info(pl, ens, -1, 2, 1, 1, info), "B < 0");
    REFUSED(gel_prop_adjoint_wind_info(pl, ens, B, 2, 2, 1, info), "shared is neither");
    REFUSED(gel_prop_adjoint_wind_info(pl, ens, B, 1 << 24, 0, 1, info), "1 GB");
    REQUIRE(gel_prop_plan_destroy(pl) == GEL_OK);
  }
  REQUIRE(gel_wind_ensemble_destroy(ens) == GEL_OK && gel_wind_ensemble_destroy(shrt) == GEL_OK && gel_wind_ensemble_destroy(foreign) == GEL_OK);
  REQUIRE(gel_wind_ensemble_destroy(unassigned) == GEL_OK && gel_wind_ensemble_destroy(small) == GEL_OK);
  REQUIRE(gel_problem_destroy(other) == GEL_OK && gel_problem_destroy(p) == GEL_OK);
  printf("FLIGHT_WIND_SANITIZE_OK\n");
  return 0;
}
