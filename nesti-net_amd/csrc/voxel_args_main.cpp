// Stand-alone driver of the voxel downsampling's host side (voxel.hip): the workspace size, the sort's tile and every argument refusal
// of nesti_voxel_keys, nesti_sort_pairs and nesti_voxel_reduce, all of which return before any device call.  Built and run by
// `make asan-voxel` against the AddressSanitizer build of the library.
#include "args_main.h"

int main() {
  const int N = 1000;
  double dummy[4] = {0.0, 0.0, 0.0, 0.0};   // never dereferenced: the checks come first
  void* p = dummy;
  char other[8];
  void* q = other;
  const size_t ws = nesti_voxel_workspace_bytes(N);

  // ---- the workspace size and the tile ---------------------------------------------------------------------------------------------------
  if (nesti_voxel_workspace_bytes(0) != 0 || nesti_voxel_workspace_bytes(-5) != 0 || ws == 0 || ws % 256 != 0 ||
      nesti_voxel_workspace_bytes(1) == 0 || nesti_voxel_workspace_bytes(1) % 256 != 0 ||
      nesti_voxel_workspace_bytes(1 << 20) <= nesti_voxel_workspace_bytes(1000) || nesti_voxel_workspace_bytes(2147483647) % 256 != 0 ||
      nesti_voxel_workspace_bytes(2147483647) < (size_t)2147483647 * 12) {
    printf("FAIL nesti_voxel_workspace_bytes\n");
    ++failures;
  }
  if (nesti_sort_tile_items() <= 0 || nesti_sort_tile_items() != nesti_sort_tile_items()) {
    printf("FAIL nesti_sort_tile_items\n");
    ++failures;
  }

  const char* name = "nesti_voxel_keys";
#define REFUSED(CALL, word, what, ...)      \
  refused(CALL(__VA_ARGS__), word, what);   \
  refused(1, name, what ": under the entry's name")

  // ---- nesti_voxel_keys --------------------------------------------------------------------------------------------------------------------
  const double o[3] = {0.0, -1.0, 2.0}, o_nan[3] = {0.0, NAN, 2.0}, o_inf[3] = {-INFINITY, 0.0, 0.0};
  const double v[3] = {0.1, 0.2, 0.3}, v_zero[3] = {0.1, 0.0, 0.3}, v_neg[3] = {-0.1, 0.2, 0.3}, v_nan[3] = {0.1, 0.2, NAN},
               v_inf[3] = {INFINITY, 0.2, 0.3};
  const int64_t d[3] = {10, 20, 30}, d_zero[3] = {10, 0, 30}, d_neg[3] = {10, 20, -1}, d_62[3] = {1ll << 31, 1ll << 31, 1},
                d_big[3] = {1ll << 40, 1ll << 40, 1ll << 40}, d_max[3] = {INT64_MAX, INT64_MAX, INT64_MAX};
#define KEYS(cloud, n, org, vox, dm, out) \
  nesti_voxel_keys((const float*)(cloud), n, (const double*)(org), (const double*)(vox), (const int64_t*)(dm), (uint64_t*)(out), NULL)
  REFUSED(KEYS, "null", "keys: null cloud", NULL, N, o, v, d, p);
  REFUSED(KEYS, "null", "keys: null origin", p, N, NULL, v, d, p);
  REFUSED(KEYS, "null", "keys: null voxel", p, N, o, NULL, d, p);
  REFUSED(KEYS, "null", "keys: null dims", p, N, o, v, NULL, p);
  REFUSED(KEYS, "null", "keys: null output", p, N, o, v, d, NULL);
  REFUSED(KEYS, "empty cloud", "keys: N = 0", p, 0, o, v, d, p);
  REFUSED(KEYS, "empty cloud", "keys: N < 0", p, -1, o, v, d, p);
  REFUSED(KEYS, "voxel sizes", "keys: voxel 0", p, N, o, v_zero, d, p);
  REFUSED(KEYS, "voxel sizes", "keys: voxel < 0", p, N, o, v_neg, d, p);
  REFUSED(KEYS, "voxel sizes", "keys: voxel NaN", p, N, o, v_nan, d, p);
  REFUSED(KEYS, "voxel sizes", "keys: voxel inf", p, N, o, v_inf, d, p);
  REFUSED(KEYS, "origin", "keys: origin NaN", p, N, o_nan, v, d, p);
  REFUSED(KEYS, "origin", "keys: origin inf", p, N, o_inf, v, d, p);
  REFUSED(KEYS, "dims must be", "keys: dims 0", p, N, o, v, d_zero, p);
  REFUSED(KEYS, "dims must be", "keys: dims < 0", p, N, o, v, d_neg, p);
  REFUSED(KEYS, "2^62", "keys: cells = 2^62", p, N, o, v, d_62, p);
  REFUSED(KEYS, "2^62", "keys: cells = 2^120", p, N, o, v, d_big, p);
  REFUSED(KEYS, "2^62", "keys: cells beyond 64 bits", p, N, o, v, d_max, p);

  // ---- nesti_sort_pairs --------------------------------------------------------------------------------------------------------------------
#define SORT(in, n, bits, kout, iout, ws_, bytes) \
  nesti_sort_pairs((const uint64_t*)(in), n, bits, (uint64_t*)(kout), (int32_t*)(iout), ws_, bytes, NULL)
  name = "nesti_sort_pairs";
  REFUSED(SORT, "null", "sort: null keys", NULL, N, 32, q, p, p, ws);
  REFUSED(SORT, "null", "sort: null keys_out", p, N, 32, NULL, p, p, ws);
  REFUSED(SORT, "null", "sort: null idx_out", p, N, 32, q, NULL, p, ws);
  REFUSED(SORT, "null", "sort: null workspace", p, N, 32, q, p, NULL, ws);
  REFUSED(SORT, "N must be", "sort: N = 0", p, 0, 32, q, p, p, ws);
  REFUSED(SORT, "N must be", "sort: N < 0", p, -7, 32, q, p, p, ws);
  REFUSED(SORT, "key_bits", "sort: key_bits 0", p, N, 0, q, p, p, ws);
  REFUSED(SORT, "key_bits", "sort: key_bits < 0", p, N, -8, q, p, p, ws);
  REFUSED(SORT, "key_bits", "sort: key_bits 65", p, N, 65, q, p, p, ws);
  REFUSED(SORT, "workspace too small", "sort: short workspace", p, N, 32, q, p, p, ws - 1);
  REFUSED(SORT, "workspace too small", "sort: no workspace bytes", p, 1, 1, q, p, p, (size_t)0);
  REFUSED(SORT, "keys_out must not be keys_in", "sort: in place", p, N, 32, p, p, p, ws);

  // ---- nesti_voxel_reduce ------------------------------------------------------------------------------------------------------------------
#define REDUCE(cloud, n, keys, idx, org, nvox, ws_, bytes)                                                                             \
  nesti_voxel_reduce((const float*)(cloud), n, (const uint64_t*)(keys), (const int32_t*)(idx), 6000, (const double*)(org), (float*)p, \
                     (int32_t*)p, (int32_t*)p, (uint64_t*)p, (int32_t*)p, (int32_t*)(nvox), ws_, bytes, NULL)
  name = "nesti_voxel_reduce";
  REFUSED(REDUCE, "null", "reduce: null cloud", NULL, N, p, p, o, p, p, ws);
  REFUSED(REDUCE, "null", "reduce: null keys", p, N, NULL, p, o, p, p, ws);
  REFUSED(REDUCE, "null", "reduce: null idx", p, N, p, NULL, o, p, p, ws);
  REFUSED(REDUCE, "null", "reduce: null origin", p, N, p, p, NULL, p, p, ws);
  REFUSED(REDUCE, "null", "reduce: null n_voxels", p, N, p, p, o, NULL, p, ws);
  REFUSED(REDUCE, "null", "reduce: null workspace", p, N, p, p, o, p, NULL, ws);
  REFUSED(REDUCE, "empty cloud", "reduce: N = 0", p, 0, p, p, o, p, p, ws);
  REFUSED(REDUCE, "empty cloud", "reduce: N < 0", p, -1, p, p, o, p, p, ws);
  REFUSED(REDUCE, "origin", "reduce: origin NaN", p, N, p, p, o_nan, p, p, ws);
  REFUSED(REDUCE, "origin", "reduce: origin inf", p, N, p, p, o_inf, p, p, ws);
  REFUSED(REDUCE, "workspace too small", "reduce: short workspace", p, N, p, p, o, p, p, ws - 1);
  // every NULL-able output NULL: still the short workspace that is refused
  refused(nesti_voxel_reduce((const float*)p, N, (const uint64_t*)p, (const int32_t*)p, 6000, o, NULL, NULL, NULL, NULL, NULL, (int32_t*)p, p,
                             ws - 1, NULL),
          "workspace too small", "reduce: outputs NULL, short workspace");
  return finish("voxel_args");
}
