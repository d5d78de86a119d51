// Stand-alone driver of the planner's entries (plan.cpp), all host code: nesti_debug_tower_ops into output arrays of exactly the
// reported sizes for every architecture, dtype, pass and a few batch sizes, every buffer inside the tower workspace, its refusals,
// and the size entries and nesti_model_describe on the same configurations.  Built and run by `make asan-plan` against the
// AddressSanitizer build of the library.
#include <vector>

#include "args_main.h"

struct Case {
  const char* name;
  nesti_config_t cfg;
  int n_towers;
  bool gate, full;   // full: the two-stage gate and the FP8 / FP6 cross terms apply (experts_n_est on the 8^3 grid)
};

static nesti_config_t config(int arch, int n_scales, int grid_n, int n_experts, const int* lo, const int* cnt) {
  nesti_config_t c;
  nesti_default_config(&c);
  c.arch = arch; c.n_scales = n_scales; c.grid_n = grid_n; c.n_experts = n_experts;
  if (grid_n == 3) c.variance = 0.111;
  for (int i = 0; lo && i < n_experts; ++i) { c.expert_scale_lo[i] = lo[i]; c.expert_scale_cnt[i] = cnt[i]; }
  return c;
}

static void fail(const Case& cs, int dtype, int tower, int batch, const char* what) {
  printf("FAIL %s dtype %d tower %d batch %d: %s ('%s')\n", cs.name, dtype, tower, batch, what, nesti_last_error());
  ++failures;
}

// one pass of one tower: counts first, then arrays of exactly those sizes (an overrun by one element is the sanitizer's to catch)
static void plan(const Case& cs, int dtype, int tower, int batch, nesti_debug_pass_t ps) {
  int nb = 0, no = 0, np = 0;
  size_t ws = 0;
  if (nesti_debug_tower_ops(&cs.cfg, dtype, tower, batch, &ps, NULL, 0, &nb, NULL, 0, &no, NULL, 0, &np, &ws) != 0 || nb < 2 || no < 1 ||
      np < 1 || ws == 0)
    return fail(cs, dtype, tower, batch, "counts");
  std::vector<nesti_debug_buf_t> bufs(nb);
  std::vector<nesti_debug_op_t> ops(no);
  std::vector<int32_t> pos(np);
  if (nesti_debug_tower_ops(&cs.cfg, dtype, tower, batch, &ps, bufs.data(), nb, &nb, ops.data(), no, &no, pos.data(), np, &np, &ws) != 0)
    return fail(cs, dtype, tower, batch, "arrays of the reported sizes");
  for (int i = 1; i < nb; ++i)
    if (bufs[i].bytes > 0 && (bufs[i].offset < 0 || (size_t)(bufs[i].offset + bufs[i].bytes) > ws)) fail(cs, dtype, tower, batch, "a buffer leaves the workspace");
  for (int k = 0; k < no; ++k)
    if (ops[k].in_buf < 0 || ops[k].in_buf >= nb || ops[k].out_buf < 1 || ops[k].out_buf >= nb) fail(cs, dtype, tower, batch, "a launch names no buffer");
  // the filter pass is what nesti_tower_workspace_bytes quotes for the gating net of the two-stage models
  const bool two_stage = dtype == NESTI_F16X3C || dtype == NESTI_F16X8C;
  if ((ps.fast || !(tower < 0 && two_stage)) && nesti_tower_workspace_bytes(&cs.cfg, dtype, tower, batch) != ws)
    fail(cs, dtype, tower, batch, "nesti_tower_workspace_bytes differs");
  refused(nesti_debug_tower_ops(&cs.cfg, dtype, tower, batch, &ps, bufs.data(), nb - 1, &nb, ops.data(), no, &no, pos.data(), np, &np, &ws),
          "too small", "bufs one too small");
  refused(nesti_debug_tower_ops(&cs.cfg, dtype, tower, batch, &ps, bufs.data(), nb, &nb, ops.data(), no - 1, &no, pos.data(), np, &np, &ws),
          "too small", "ops one too small");
  refused(nesti_debug_tower_ops(&cs.cfg, dtype, tower, batch, &ps, bufs.data(), nb, &nb, ops.data(), no, &no, pos.data(), np - 1, &np, &ws),
          "too small", "in_pos one too small");
}

int main() {
  const int one_lo[1] = {0}, one_cnt[1] = {1}, all_cnt[1] = {3}, sw_lo[2] = {0, 1}, sw_cnt[2] = {1, 1};
  const Case cases[] = {
      {"experts", config(NESTI_ARCH_EXPERTS, 3, 8, 7, NULL, NULL), 7, true, true},
      {"grid3", config(NESTI_ARCH_EXPERTS, 3, 3, 7, NULL, NULL), 7, true, false},
      {"ss_norm_est", config(NESTI_ARCH_SINGLE, 1, 8, 1, one_lo, one_cnt), 1, false, false},
      {"ms_norm_est", config(NESTI_ARCH_MULTI, 3, 8, 1, one_lo, all_cnt), 1, false, false},
      {"ms_sw_n_est", config(NESTI_ARCH_SWITCH, 2, 8, 2, sw_lo, sw_cnt), 2, true, false},
  };
  const int batches[] = {1, 37, 100000};
  for (const Case& cs : cases) {
    for (int dtype = NESTI_F32; dtype <= (cs.full ? NESTI_F16X8C : NESTI_F16X3); ++dtype) {
      const bool two_stage = dtype == NESTI_F16X3C || dtype == NESTI_F16X8C, x8 = dtype == NESTI_F16X8 || dtype == NESTI_F16X8C;
      for (int batch : batches) {
        for (int tower = cs.gate ? -1 : 0; tower < cs.n_towers; ++tower) {
          plan(cs, dtype, tower, batch, {0, 0, 0});
          if (tower < 0 && two_stage) plan(cs, dtype, tower, batch, {1, 0, 0});
          if (tower >= 0 && x8)
            for (int fmt : {6, 8}) plan(cs, dtype, tower, batch, {0, 0xF, fmt});
        }
        if (nesti_estimate_workspace_bytes_for_config(&cs.cfg, dtype, batch) == 0) fail(cs, dtype, 0, batch, "nesti_estimate_workspace_bytes_for_config");
      }
      if (nesti_tower_workspace_bytes(&cs.cfg, dtype, cs.n_towers, 37) != 0 || nesti_tower_workspace_bytes(&cs.cfg, dtype, 0, 0) != 0 ||
          nesti_estimate_workspace_bytes_for_config(&cs.cfg, dtype, 0) != 0)
        fail(cs, dtype, cs.n_towers, 0, "a size entry accepts a bad tower or batch");
    }
    int n = 0;
    if (nesti_model_describe(&cs.cfg, &n, NULL, 0) != 0 || n < 1) { fail(cs, 0, 0, 0, "nesti_model_describe: count"); continue; }
    std::vector<nesti_tensor_t> infos(n);
    if (nesti_model_describe(&cs.cfg, &n, infos.data(), n) != 0 || !infos[n - 1].name) fail(cs, 0, 0, 0, "nesti_model_describe");
    refused(nesti_model_describe(&cs.cfg, &n, infos.data(), n - 1), "too small", "describe: infos one too small");
  }

  const nesti_config_t* cfg = &cases[0].cfg;
  int nb = 0, no = 0;
  nesti_debug_pass_t ps = {1, 0, 0};
#define OPS(c, dtype, tower, batch, pass) nesti_debug_tower_ops(c, dtype, tower, batch, pass, NULL, 0, &nb, NULL, 0, &no, NULL, 0, NULL, NULL)
  refused(OPS(NULL, NESTI_F16, 0, 8, NULL), "null", "null config");
  refused(nesti_debug_tower_ops(cfg, NESTI_F16, 0, 8, NULL, NULL, 0, NULL, NULL, 0, &no, NULL, 0, NULL, NULL), "null", "null n_bufs");
  refused(OPS(cfg, NESTI_F16, 0, 0, NULL), "batch", "batch = 0");
  refused(OPS(cfg, NESTI_F16, 0, -5, NULL), "batch", "batch < 0");
  refused(OPS(cfg, NESTI_F16X3, -1, 8, &ps), "filter pass", "filter pass without the two-stage gate");
  refused(OPS(cfg, NESTI_F16X3C, 0, 8, &ps), "filter pass", "filter pass on an expert");
  refused(OPS(cfg, NESTI_F16, 7, 8, NULL), "tower", "tower = E");
  refused(OPS(cfg, NESTI_F16, -2, 8, NULL), "tower", "tower = -2");
  refused(OPS(&cases[2].cfg, NESTI_F16, -1, 8, NULL), "no gating net", "gate of a single-tower model");
  ps = {0, 0x10, 6};
  refused(OPS(cfg, NESTI_F16X8C, 0, 8, &ps), "x8_mask", "x8_mask with five bits");
  ps = {0, -1, 6};
  refused(OPS(cfg, NESTI_F16X8C, 0, 8, &ps), "x8_mask", "x8_mask < 0");
  ps = {0, 0xF, 6};
  refused(OPS(cfg, NESTI_F16X8C, -1, 8, &ps), "x8_mask", "x8_mask on the gating net");
  refused(OPS(cfg, NESTI_F16X3C, 0, 8, &ps), "x8_mask", "x8_mask without the cross-term side buffers");
  ps = {0, 0xF, 7};
  refused(OPS(cfg, NESTI_F16X8C, 0, 8, &ps), "x8_fmt", "x8_fmt = 7");
  return finish("plan_args");
}
