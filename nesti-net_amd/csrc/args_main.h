// What the stand-alone drivers of the entries' host side (*_args_main.cpp, built and run by `make asan-<name>` against the
// AddressSanitizer build of the library) share: the failure count, the check of a refusal, the refusals of the ball-fit entries and
// the final line.
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../include/nesti_hip.h"

static int failures = 0;

// the call was refused (rc != 0) and the message names `word`
static void refused(int rc, const char* word, const char* what) {
  const char* msg = nesti_last_error();
  if (rc == 0 || !msg || !strstr(msg, word)) {
    printf("FAIL %s: rc %d, message '%s'\n", what, rc, msg ? msg : "(null)");
    ++failures;
  }
}

// What a pair of ball-fit entries (nesti_pca_normals / _at, nesti_quadric_fit / _at) refuses before any device call, and that M = 0
// is a no-op.  idx(cfg, cloud, N, query_idx, M, r_abs, query_row0, grid_ws, grid_ws_bytes) calls the index form and at(...) the
// positions form with any non-null outputs; the pointers are never dereferenced, the checks come first.  Ends with a refusal of
// the positions form, so nesti_last_error() names that entry on return.
template <class Idx, class At>
static void ball_fit_refusals(Idx&& idx, At&& at) {
  const int N = 1000, M = 100;
  float dummy[4] = {0.f, 0.f, 0.f, 0.f};
  const void* p = dummy;
  nesti_config_t cfg;
  nesti_default_config(&cfg);
  const size_t gws = nesti_patches_workspace_bytes(N);
  const double r[4] = {0.01, 0.03, 0.05, 0.07}, r_zero[4] = {0.01, 0.0, 0.05, 0.07}, r_neg[4] = {-0.01, 0.03, 0.05, 0.07},
               r_nan[4] = {0.01, 0.03, NAN, 0.07}, r_inf[4] = {INFINITY, 0.03, 0.05, 0.07};
  nesti_config_t none = cfg, many = cfg;
  none.n_scales = 0;
  many.n_scales = NESTI_MAX_SCALES + 1;
  const struct {
    const char *word, *what;
    const nesti_config_t* c;
    const void* cloud;
    int n, m;
    const double* rad;
    int row0;
    const void* g;
    size_t gb;
  } both[] = {
      {"null", "null config", NULL, p, N, M, r, 0, p, gws},
      {"null", "null cloud", &cfg, NULL, N, M, r, 0, p, gws},
      {"null", "null radii", &cfg, p, N, M, NULL, 0, p, gws},
      {"null", "null grid workspace", &cfg, p, N, M, r, 0, NULL, gws},
      {"empty cloud", "N = 0", &cfg, p, 0, M, r, 0, p, gws},
      {"M must be", "M < 0", &cfg, p, N, -1, r, 0, p, gws},
      {"workspace too small", "short grid workspace", &cfg, p, N, M, r, 0, p, gws - 1},
      {"query_row0", "query_row0 < 0", &cfg, p, N, M, r, -1, p, gws},
      {"radii", "radius 0", &cfg, p, N, M, r_zero, 0, p, gws},
      {"radii", "radius < 0", &cfg, p, N, M, r_neg, 0, p, gws},
      {"radii", "radius NaN", &cfg, p, N, M, r_nan, 0, p, gws},
      {"radii", "radius inf", &cfg, p, N, M, r_inf, 0, p, gws},
      {"n_scales", "S = 0", &none, p, N, M, r, 0, p, gws},
      {"n_scales", "S = NESTI_MAX_SCALES + 1", &many, p, N, M, r, 0, p, gws},
  };
  char what[96];
  for (const auto& b : both) {
    snprintf(what, sizeof(what), "index: %s", b.what);
    refused(idx(b.c, (const float*)b.cloud, b.n, (const int32_t*)p, b.m, b.rad, b.row0, b.g, b.gb), b.word, what);
    snprintf(what, sizeof(what), "positions: %s", b.what);
    refused(at(b.c, (const float*)b.cloud, b.n, (const float*)p, b.m, b.rad, b.row0, b.g, b.gb), b.word, what);
  }
  const float* cloud = (const float*)p;
  // M = 0 is a no-op, and an argument error is still one
  if (idx(&cfg, cloud, N, NULL, 0, r, 0, p, gws) != 0 || at(&cfg, cloud, N, NULL, 0, r, 0, p, gws) != 0) {
    printf("FAIL M = 0 is a no-op\n");
    ++failures;
  }
  refused(idx(&cfg, cloud, N, NULL, 0, r_nan, 0, p, gws), "radii", "index: M = 0 with a NaN radius");
  refused(idx(&cfg, cloud, N, NULL, M, r, N - M + 1, p, gws), "exceed the cloud", "index: rows beyond the cloud");
  refused(at(&cfg, cloud, N, NULL, M, r, 0, p, gws), "null query_xyz_dev", "positions: null positions");
}

// The lane switch of a list pass (nesti_debug_smooth_lanes, _denoise_lanes, _outlier_lanes): a value that is no lane group is
// refused under the entry's name, 16, 32 and 64 are accepted, and 0 -- the default, set last -- too.
static void lane_switch_refusals(int (*entry)(int), const char* name) {
  char what[96];
  const int bad_lanes[] = {-1, 1, 8, 48, 128};
  for (int lanes : bad_lanes) {
    snprintf(what, sizeof(what), "%s(%d): a lane group that is none", name, lanes);
    refused(entry(lanes), "lanes must be", what);
    refused(1, name, what);
  }
  const int good_lanes[] = {16, 32, 64, 0};
  for (int lanes : good_lanes)
    if (entry(lanes) != 0) {
      printf("FAIL %s(%d): '%s'\n", name, lanes, nesti_last_error());
      ++failures;
    }
}

// prints "<name>: ok" or the number of failures; the value main() returns
static int finish(const char* name) {
  if (failures) printf("%s: %d failure(s)\n", name, failures);
  else printf("%s: ok\n", name);
  return failures ? 1 : 0;
}
