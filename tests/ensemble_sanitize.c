/* The wind ensemble's host code under AddressSanitizer + UBSan (CPU build only; nothing is launched): create on a host-only
 * handle, gel_wind_ensemble_member into exactly sized heap buffers against the slopes restated here, info, assign and re-assign,
 * every refusal (sizes, a member whose altitudes do not increase, a NaN altitude, member = E and -2, an assignment that does not
 * match the call, an ensemble of another handle), the evaluation calls' refusal of a host-only handle, destroy.  Prints
 * ENSEMBLE_SANITIZE_OK on success. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/gelato_amd.h"

#define REQUIRE(c)                                                          \
  do {                                                                      \
    if (!(c)) { fprintf(stderr, "REQUIRE failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, gel_last_error()); return 1; } \
  } while (0)

static gel_problem* host_problem(void) {
  enum { S = 3 };
  static const int32_t nn[S] = {2, 3, 4};
  static const double thrust[S] = {420000.0, 0.0, 30700.0};
  static const double mdot[S] = {140.0, 0.0, 9.8};
  static const double area[S] = {2.21, 2.21, 0.0};
  static const double nozzle[S] = {0.68, 0.0, 0.0};
  static const int32_t on[S] = {1, 0, 1};
  static const int32_t hold[S] = {1, 0, 0};
  static const double wind[3][3] = {{0.0, 1.0, 2.0}, {5000.0, 3.0, -1.0}, {20000.0, 10.0, 4.0}};
  static const double ca[2][2] = {{0.0, 0.3}, {5.0, 0.5}};
  gel_problem_desc d;
  memset(&d, 0, sizeof d);
  d.num_sections = S; d.num_nodes = nn; d.thrust = thrust; d.massflow = mdot; d.reference_area = area;
  d.nozzle_area = nozzle; d.engine_on = on; d.attitude_hold = hold;
  d.unit_mass = 27442.0; d.unit_position = 6378137.0; d.unit_velocity = 1000.0; d.unit_u = 1.0; d.unit_t = 597.0;
  d.dx = 1e-8; d.wind_rows = 3; d.wind_table = &wind[0][0]; d.ca_rows = 2; d.ca_table = &ca[0][0];
  d.device = GEL_DEVICE_NONE;
  gel_problem* p = NULL;
  return gel_problem_create(&d, &p) == GEL_OK ? p : NULL;
}

int main(void) {
  gel_problem* p = host_problem();
  gel_problem* other = host_problem();
  REQUIRE(p && other);

  enum { E = 5, Kw = 37 };
  double* t = malloc(sizeof(double) * E * Kw * 3);
  for (int e = 0; e < E; e++)
    for (int k = 0; k < Kw; k++) {
      double* r = t + ((size_t)e * Kw + k) * 3;
      r[0] = 100.0 * e + 731.0 * k + 0.37 * k * k;          /* every member its own altitudes */
      r[1] = 30.0 * sin(0.3 * k + e);
      r[2] = (e == 2) ? 0.0 : -20.0 * cos(0.2 * k - e);
    }
  gel_wind_ensemble* ens = NULL;
  REQUIRE(gel_wind_ensemble_create(p, E, Kw, t, &ens) == GEL_OK && ens);
  int64_t info[5];
  REQUIRE(gel_wind_ensemble_info(ens, info) == GEL_OK);
  REQUIRE(info[0] == E && info[1] == Kw && info[2] == 5 * Kw - 2 && info[3] == 0 && info[4] == -1);
  for (int e = 0; e < E; e++) {
    double* st = malloc(sizeof(double) * (5 * Kw - 2));
    REQUIRE(gel_wind_ensemble_member(ens, e, st) == GEL_OK);
    const double* r = t + (size_t)e * Kw * 3;
    REQUIRE(memcmp(st, r, sizeof(double) * 3 * Kw) == 0);
    for (int k = 0; k + 1 < Kw; k++)
      for (int c = 1; c < 3; c++) {
        const double s = (r[3 * (k + 1) + c] - r[3 * k + c]) / (r[3 * (k + 1)] - r[3 * k]);
        REQUIRE(memcmp(&s, st + 3 * Kw + 2 * k + (c - 1), sizeof s) == 0);
      }
    free(st);
  }
  double one[1];
  REQUIRE(gel_wind_ensemble_member(ens, E, one) == GEL_ERR_ARG && gel_wind_ensemble_member(ens, -1, one) == GEL_ERR_ARG);
  REQUIRE(gel_wind_ensemble_member(ens, 0, NULL) == GEL_ERR_ARG);

  /* assign: validated on the host; a host-only handle keeps the count */
  enum { B = 67 };
  int32_t* m = malloc(sizeof(int32_t) * B);
  for (int b = 0; b < B; b++) m[b] = b % (E + 1) - 1;
  REQUIRE(gel_wind_ensemble_assign(ens, B, m) == GEL_OK);
  REQUIRE(gel_wind_ensemble_info(ens, info) == GEL_OK && info[4] == B);
  m[40] = E;
  REQUIRE(gel_wind_ensemble_assign(ens, B, m) == GEL_ERR_ARG && strstr(gel_last_error(), "member[40] = 5"));
  m[40] = 0; m[3] = -2;
  REQUIRE(gel_wind_ensemble_assign(ens, B, m) == GEL_ERR_ARG && strstr(gel_last_error(), "member[3] = -2"));
  REQUIRE(gel_wind_ensemble_info(ens, info) == GEL_OK && info[4] == B);      /* a refused assignment leaves the old one */
  m[3] = -1;
  REQUIRE(gel_wind_ensemble_assign(ens, -1, m) == GEL_ERR_ARG && gel_wind_ensemble_assign(ens, 1, NULL) == GEL_ERR_ARG);
  REQUIRE(gel_wind_ensemble_assign(NULL, 1, m) == GEL_ERR_ARG);
  REQUIRE(gel_wind_ensemble_assign(ens, 3, m) == GEL_OK && gel_wind_ensemble_info(ens, info) == GEL_OK && info[4] == 3);
  REQUIRE(gel_wind_ensemble_assign(ens, 0, NULL) == GEL_OK && gel_wind_ensemble_info(ens, info) == GEL_OK && info[4] == 0);
  REQUIRE(gel_wind_ensemble_assign(ens, 3, m) == GEL_OK);

  /* the evaluation calls: the ensemble's checks come before the device is looked at, a host-only handle never evaluates */
  const int32_t steps[3] = {1, 2, 1};
  gel_prop_plan *pl = NULL, *pl_other = NULL;
  REQUIRE(gel_prop_plan_create(p, steps, GEL_PROP_CHAIN, &pl) == GEL_OK && gel_prop_plan_create(other, steps, 0, &pl_other) == GEL_OK);
  double x[1] = {0.0}, y[1], f[1] = {1.0};
  REQUIRE(gel_propagate_ensemble(pl, 3, x, f, ens, y, NULL) == GEL_ERR_HIP);
  REQUIRE(gel_propagate_ensemble_device(pl, 3, x, NULL, ens, y, NULL) == GEL_ERR_HIP);
  REQUIRE(gel_propagate_ensemble(pl, 3, x, f, NULL, y, NULL) == GEL_ERR_HIP);
  REQUIRE(gel_propagate_ensemble(pl, 4, x, f, ens, y, NULL) == GEL_ERR_ARG && strstr(gel_last_error(), "assigned 3 vectors"));
  REQUIRE(gel_propagate_ensemble_device(pl, 2, x, f, ens, y, NULL) == GEL_ERR_ARG);
  REQUIRE(gel_propagate_ensemble(pl_other, 3, x, f, ens, y, NULL) == GEL_ERR_ARG && strstr(gel_last_error(), "another handle"));
  REQUIRE(gel_propagate_ensemble_device(pl_other, 3, x, f, ens, y, NULL) == GEL_ERR_ARG);
  REQUIRE(gel_propagate_ensemble(pl, -1, x, f, ens, y, NULL) == GEL_ERR_ARG && gel_propagate_ensemble(pl, 3, NULL, f, ens, y, NULL) == GEL_ERR_ARG);
  REQUIRE(gel_output_table_batch_ensemble(p, 3, x, NULL, NULL, ens, 0.0, 0.0, 0, NULL, y, NULL, NULL) == GEL_ERR_HIP);
  REQUIRE(gel_output_table_batch_ensemble_device(p, 3, x, NULL, NULL, ens, 0.0, 0.0, 0, NULL, y, NULL, NULL) == GEL_ERR_HIP);
  REQUIRE(gel_output_table_batch_ensemble(p, 5, x, NULL, NULL, ens, 0.0, 0.0, 0, NULL, y, NULL, NULL) == GEL_ERR_ARG);
  REQUIRE(gel_output_table_batch_ensemble_device(other, 3, x, NULL, NULL, ens, 0.0, 0.0, 0, NULL, y, NULL, NULL) == GEL_ERR_ARG &&
          strstr(gel_last_error(), "another handle"));
  REQUIRE(gel_output_table_batch_ensemble(p, 3, x, NULL, NULL, ens, 0.0, 0.0, 0, NULL, NULL, NULL, NULL) == GEL_ERR_ARG);
  REQUIRE(gel_prop_plan_destroy(pl) == GEL_OK && gel_prop_plan_destroy(pl_other) == GEL_OK);

  /* refusals of create */
  gel_wind_ensemble* q = NULL;
  REQUIRE(gel_wind_ensemble_create(p, 0, Kw, t, &q) == GEL_ERR_ARG && q == NULL && strstr(gel_last_error(), "E = 0"));
  REQUIRE(gel_wind_ensemble_create(p, E, 1, t, &q) == GEL_ERR_ARG && q == NULL && strstr(gel_last_error(), "Kw = 1"));
  REQUIRE(gel_wind_ensemble_create(NULL, E, Kw, t, &q) == GEL_ERR_ARG && gel_wind_ensemble_create(p, E, Kw, t, NULL) == GEL_ERR_ARG);
  REQUIRE(gel_wind_ensemble_create(p, E, Kw, NULL, &q) == GEL_ERR_ARG && strstr(gel_last_error(), "tables is NULL"));
  /* sizes only: E (5 Kw - 2) = 2^27 with Kw = 26 (128 doubles per member), E = 2^20 is the limit; a null table is what is refused there */
  REQUIRE(gel_wind_ensemble_create(p, 1 << 20, 26, NULL, &q) == GEL_ERR_ARG && strstr(gel_last_error(), "tables is NULL"));
  REQUIRE(gel_wind_ensemble_create(p, (1 << 20) + 1, 26, NULL, &q) == GEL_ERR_ARG && strstr(gel_last_error(), "2^27"));
  REQUIRE(gel_wind_ensemble_create(p, 1, 1 << 20, NULL, &q) == GEL_ERR_ARG && strstr(gel_last_error(), "tables is NULL"));
  REQUIRE(gel_wind_ensemble_create(p, 1, (1 << 20) + 1, NULL, &q) == GEL_ERR_ARG && strstr(gel_last_error(), "2^20"));
  const double keep = t[((size_t)3 * Kw + 9) * 3];
  t[((size_t)3 * Kw + 9) * 3] = t[((size_t)3 * Kw + 8) * 3];                  /* member 3: two equal altitudes */
  REQUIRE(gel_wind_ensemble_create(p, E, Kw, t, &q) == GEL_ERR_ARG && q == NULL && strstr(gel_last_error(), "member 3") &&
          strstr(gel_last_error(), "increase strictly"));
  t[((size_t)3 * Kw + 9) * 3] = NAN;
  REQUIRE(gel_wind_ensemble_create(p, E, Kw, t, &q) == GEL_ERR_ARG && q == NULL && strstr(gel_last_error(), "member 3"));
  t[((size_t)3 * Kw + 9) * 3] = keep;
  t[1] = NAN;                                                                  /* a NaN WIND entry is data, not a refusal */
  REQUIRE(gel_wind_ensemble_create(p, E, Kw, t, &q) == GEL_OK && q);
  REQUIRE(gel_wind_ensemble_destroy(q) == GEL_OK);

  REQUIRE(gel_wind_ensemble_destroy(ens) == GEL_OK && gel_wind_ensemble_destroy(NULL) == GEL_OK);
  free(m); free(t);
  REQUIRE(gel_problem_destroy(p) == GEL_OK && gel_problem_destroy(other) == GEL_OK);
  printf("ENSEMBLE_SANITIZE_OK\n");
  return 0;
}
