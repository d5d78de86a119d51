// Graph builder: the towers of experts_n_est and of the ablation models as buffers and launches (graph.h).  Host only.
#include <functional>

#include "graph.h"

namespace nesti {
namespace {

constexpr int kPad = 64;   // channel segments are zero-padded to multiples of this
inline int pad_to(int c, int a) { return (c + a - 1) / a * a; }

struct Builder {
  Graph& g;
  bool x8 = false;           // expert towers of an NESTI_F16X8 / NESTI_F16X8C model: side buffers for the 8^3 blocks' tap layers
  int x8_block = 0;          // ... and which 8^3 inception block of the tower is being built (0, 1)
  int s_real = 0;            // stamped on the layers built while it is set (conv_net_3g)
  explicit Builder(Graph& gg) : g(gg) {}

  int add_layer(const LayerDesc& d) { g.layers.push_back(d); return (int)g.layers.size() - 1; }

  int conv(Tower& T, const std::string& scope, int k, int log2S, int in_buf, int in_coff, const ChanMap& in,
           int cout, int out_buf, int out_coff, bool bn = true, bool relu = true, bool fc = false, bool out_f32 = false,
           const std::string& scope2 = "", int out_coff2 = 0, int pool_k = 1) {
    LayerDesc d;
    d.scope = scope; d.scope2 = scope2; d.pool_k = pool_k; d.is_fc = fc; d.k = k; d.log2S = log2S;
    d.s_real = fc ? 0 : s_real;
    d.cin = (int)in.pos.size(); d.cout = cout; d.in_pos = in.pos; d.Cin_p = in.C;
    d.Cout_p = pad_to(cout, kPad) * (scope2.empty() ? 1 : 2); d.bn = bn; d.relu = relu;
    Op op; op.kind = Op::CONV; op.in_buf = in_buf; op.in_coff = in_coff; op.out_buf = out_buf; op.out_coff = out_coff;
    op.out_coff2 = out_coff2;
    op.layer = add_layer(d); op.log2S = log2S; op.out_f32 = out_f32;
    T.ops.push_back(op);
    return d.Cout_p;
  }

  // models/experts_n_est.py:294-314.  conv1 and conv4 read the same tensor (avg_pool3d commutes with the
  // 1x1x1 convolution), so they are one launch; conv4's columns are averaged in the kernel epilogue.
  // then_maxpool: the block is followed by tf_util.max_pool3d 2^3/2 (e.g. models/experts_n_est.py:198).  conv1
  // stores full resolution (conv2/conv3 read it) AND its pooled tensor, conv2/conv3 store only the pooled tensor
  // (nobody reads them at full resolution); conv4's columns come out of the avg-pool epilogue at full resolution
  // and are max-pooled by the small standalone kernel, restricted to their channel range.  Returns the buffer the
  // next block reads.
  int inception(Tower& T, const std::string& scope, int in_buf, const ChanMap& in, int F, int k0, int k1, int log2S,
                ChanMap* out_map, bool then_maxpool = false) {
    const int H = F / 2;   // int(n_filters/2)  :299
    const int Fp = pad_to(F, kPad), Hp = pad_to(H, kPad);
    const int C = Fp + Hp + Hp + Fp;
    T.bufs.push_back({log2S, C, false});
    const int ob = (int)T.bufs.size() - 1;
    int pb = -1;
    if (then_maxpool) {
      T.bufs.push_back({log2S - 1, C, false});
      pb = (int)T.bufs.size() - 1;
    }
    ChanMap c1; c1.C = Fp; for (int i = 0; i < F; ++i) c1.pos.push_back(i);
    conv(T, scope + "_conv1", 1, log2S, in_buf, 0, in, F, ob, 0, true, true, false, false,
         scope + "_conv4", Fp + Hp + Hp, k0);
    // conv4 behind a max-pool: when its avg-pool runs in the epilogue (k0 > 1) the 2^3 max is taken there as well and
    // its full-resolution columns are never written; with k0 == 1 (plain columns) the small standalone kernel pools them
    const bool fuse4 = then_maxpool && k0 > 1 && !s_real;
    if (then_maxpool) { T.ops.back().mp_buf = pb; T.ops.back().mp_mode = 2; T.ops.back().mp_mode2 = fuse4 ? 1 : 0; }
    const size_t conv1_op = T.ops.size() - 1;
    int ab = -1;
    if (x8 && log2S == 3 && !s_real && x8_block < 2 && (k0 == 3 || k0 == 5) && (k1 == 3 || k1 == 5)) {
      BufSpec ax{log2S, Fp, false};
      ax.aux8 = true;
      T.bufs.push_back(ax);
      ab = (int)T.bufs.size() - 1;
      T.ops[conv1_op].aux_out_buf = ab;
      T.ops[conv1_op].x8_bits = 3 << (2 * x8_block);
    }
    conv(T, scope + "_conv2", k0, log2S, ob, 0, c1, H, ob, Fp);
    if (then_maxpool) { T.ops.back().mp_buf = pb; T.ops.back().mp_mode = 1; }
    if (ab >= 0) { T.ops.back().aux_in_buf = ab; T.ops.back().x8_bit = 2 * x8_block; T.ops.back().aux_layer = T.ops[conv1_op].layer; }
    conv(T, scope + "_conv3", k1, log2S, ob, 0, c1, H, ob, Fp + Hp);
    if (then_maxpool) { T.ops.back().mp_buf = pb; T.ops.back().mp_mode = 1; }
    if (ab >= 0) { T.ops.back().aux_in_buf = ab; T.ops.back().x8_bit = 2 * x8_block + 1; T.ops.back().aux_layer = T.ops[conv1_op].layer; ++x8_block; }
    out_map->pos.clear();
    for (int i = 0; i < F; ++i) out_map->pos.push_back(i);
    for (int i = 0; i < H; ++i) out_map->pos.push_back(Fp + i);
    for (int i = 0; i < H; ++i) out_map->pos.push_back(Fp + Hp + i);
    for (int i = 0; i < F; ++i) out_map->pos.push_back(Fp + Hp + Hp + i);
    out_map->C = C;
    if (then_maxpool) {
      if (!fuse4) {
        Op op; op.kind = Op::MAX; op.in_buf = ob; op.out_buf = pb; op.in_coff = op.out_coff = Fp + Hp + Hp;
        op.C = Fp; op.log2S = log2S;
        T.ops.push_back(op);
      }
      return pb;
    }
    return ob;
  }

  // fully connected stack on a [NB,1,C] feature (utils/tf_util.py:314-351)
  int fc_stack(Tower& T, int in_buf, ChanMap m, const std::vector<std::string>& scopes, const std::vector<int>& widths,
               bool last_relu, int first_in_cstride = 0) {
    int buf = in_buf;
    for (size_t i = 0; i < scopes.size(); ++i) {
      const bool last = (i + 1 == scopes.size());
      const int Cp = pad_to(widths[i], kPad);
      T.bufs.push_back({0, Cp, last});
      const int ob = (int)T.bufs.size() - 1;
      conv(T, scopes[i], 1, 0, buf, 0, m, widths[i], ob, 0, /*bn=*/!last, /*relu=*/last ? last_relu : true, /*fc=*/true,
           /*out_f32=*/last);
      if (i == 0) T.ops.back().in_cstride = first_in_cstride;
      m.pos.clear(); m.C = Cp;
      for (int c = 0; c < widths[i]; ++c) m.pos.push_back(c);
      buf = ob;
    }
    return buf;
  }

  void init_tower(Tower& T) {
    T.bufs.clear(); T.ops.clear();
    T.bufs.push_back({g.cfg.grid_n == 3 ? 2 : 3, g.mups_cstride, false});   // 0: X0 (3^3 grid: rows in a 4^3 index space)
  }

  // conv_net_3g (models/experts_n_est.py:217-240): four inception blocks on the 3^3 grid (kernel sizes [2,3], [2,3],
  // [1,2], [1,2]; k0 = 1 makes conv2 a 1x1x1 layer and the avg-pool of the conv4 branch the identity), then
  // max_pool3d [3,3,3] stride 2 SAME -> 2^3 x 1536, flattened voxel-major.  The 27 voxels live in a 4^3 index space
  // (host.h: ConvParams::s_real).  Returns the pooled buffer; *flat describes it as one FC input row.
  int conv_net_3g(Tower& T, const std::string& s, ChanMap m, ChanMap* flat) {
    s_real = 3;
    int b = inception(T, "inception1" + s, 0, m, 128, 2, 3, 2, &m);
    b = inception(T, "inception2" + s, b, m, 256, 2, 3, 2, &m);
    b = inception(T, "inception3" + s, b, m, 256, 1, 2, 2, &m);
    b = inception(T, "inception4" + s, b, m, 512, 1, 2, 2, &m);
    s_real = 0;
    T.bufs.push_back({1, m.C, false});
    const int pb = (int)T.bufs.size() - 1;
    Op op; op.kind = Op::MAX3; op.in_buf = b; op.out_buf = pb; op.in_coff = op.out_coff = 0; op.C = m.C; op.log2S = 2;
    T.ops.push_back(op);                                                    // maxpool5  :238
    flat->pos.clear(); flat->C = 8 * m.C;
    for (int v = 0; v < 8; ++v)
      for (size_t c = 0; c < m.pos.size(); ++c) flat->pos.push_back(v * m.C + m.pos[c]);
    return pb;
  }

  // scale_manager_net + conv_net_8g (models/experts_n_est.py:155-215)
  void build_gate() {
    Tower& T = g.gate;
    init_tower(T);
    const int S = g.cfg.n_scales;
    ChanMap m; m.C = g.mups_cstride;
    for (int c = 0; c < 20 * S; ++c) m.pos.push_back(c);
    const std::string s = "gating_conv";
    if (g.cfg.grid_n == 3) {   // models/experts_n_est.py:162-163
      ChanMap flat;
      const int pb = conv_net_3g(T, s, m, &flat);
      T.out_buf = fc_stack(T, pb, flat, {"fc1noise", "fc2noise", "fc3noise", "fc4noise"}, {1024, 256, 128, g.cfg.n_experts},
                           /*last_relu=*/true, flat.C);
      T.n_out = g.cfg.n_experts;
      return;
    }
    int b = inception(T, "inception1" + s, 0, m, 128, 3, 5, 3, &m);
    b = inception(T, "inception2" + s, b, m, 256, 3, 5, 3, &m);
    b = inception(T, "inception3" + s, b, m, 256, 3, 5, 3, &m, true);    // + maxpool4  :198
    b = inception(T, "inception5" + s, b, m, 512, 2, 4, 2, &m);
    b = inception(T, "inception6" + s, b, m, 512, 2, 4, 2, &m, true);    // + maxpool7  :206
    b = inception(T, "inception8" + s, b, m, 512, 1, 2, 1, &m, true);    // + maxpool9  :211
    T.out_buf = fc_stack(T, b, m, {"fc1noise", "fc2noise", "fc3noise", "fc4noise"}, {1024, 256, 128, g.cfg.n_experts},
                         /*last_relu=*/true);   // relu on fc4: models/experts_n_est.py:174
    T.n_out = g.cfg.n_experts;
  }

  // The stage-2 form of the gating net on the 8^3 grid (graph.h: Graph::gate2): a copy of `gate` whose 8^3 blocks' conv1 | conv4
  // launches are producers and whose 8^3 tap layers read the planes, like build_expert's first two blocks
  void build_gate2() {
    Tower& T = g.gate2;
    T = g.gate;
    T.side_tail = true;
    int block = 0, ab = -1, producer = -1;
    for (size_t k = 0; k < T.ops.size(); ++k) {
      Op& op = T.ops[k];
      if (op.kind != Op::CONV || op.log2S != 3) continue;
      const LayerDesc& d = g.layers[op.layer];
      if (!d.scope2.empty()) {   // conv1 | conv4 of an 8^3 block
        BufSpec ax{3, d.Cout_p / 2, false};
        ax.aux8 = true;
        T.bufs.push_back(ax);
        ab = (int)T.bufs.size() - 1;
        op.aux_out_buf = ab;
        op.x8_bits = 3 << (2 * block);
        producer = op.layer;
      } else if (ab >= 0 && (d.k == 3 || d.k == 5)) {
        op.aux_in_buf = ab;
        op.aux_layer = producer;
        op.x8_bit = 2 * block + (d.scope.back() == '3' ? 1 : 0);
        if (d.scope.back() == '3') { ++block; ab = -1; }
      }
    }
  }

  // The "ss" tower shared by the ablation models: inception x3 @8^3 [3,5] -> maxpool -> inception x2 @4^3
  // [3,k1_small] -> maxpool -> flatten 2^3 x 1536 voxel-major (tf.reshape) -> fc 1024/256/128/n_out.  Used by
  // ss_norm_est.get_model (models/ss_norm_est.py:35-92), ms_norm_est.get_model (models/ms_norm_est.py:45-140) and
  // the three towers of ms_sw_n_est (models/ms_sw_n_est.py:139-215).  Dropout is the identity at inference.  fc1
  // is an FC over a flattened view of the pooled buffer.
  void build_ss_tower(Tower& T, int scale_lo, int scale_cnt, const std::function<std::string(int)>& name,
                      const std::string& fc_suffix, int n_out, bool last_relu, int k1_small) {
    init_tower(T);
    ChanMap m; m.C = g.mups_cstride;
    for (int c = 0; c < 20 * scale_cnt; ++c) m.pos.push_back(20 * scale_lo + c);
    int b = inception(T, name(1), 0, m, 128, 3, 5, 3, &m);
    b = inception(T, name(2), b, m, 256, 3, 5, 3, &m);
    b = inception(T, name(3), b, m, 256, 3, 5, 3, &m, true);
    b = inception(T, name(5), b, m, 512, 3, k1_small, 2, &m);
    b = inception(T, name(6), b, m, 512, 3, k1_small, 2, &m, true);
    ChanMap flat; flat.C = 8 * m.C;
    for (int v = 0; v < 8; ++v)
      for (size_t c = 0; c < m.pos.size(); ++c) flat.pos.push_back(v * m.C + m.pos[c]);
    T.out_buf = fc_stack(T, b, flat, {"fc1" + fc_suffix, "fc2" + fc_suffix, "fc3" + fc_suffix, "fc4" + fc_suffix},
                         {1024, 256, 128, n_out}, last_relu, flat.C);
    T.n_out = n_out;
  }

  // ss_norm_est (one scale, 4^3 kernels [3,5], scopes 'inception<L>') / ms_norm_est (S scales concatenated on
  // channels, 4^3 kernels [3,4], scopes 'inception_s<S-1>_l_<L>')
  void build_single() {
    const bool multi = g.cfg.arch == NESTI_ARCH_MULTI;
    const int S = g.cfg.n_scales;
    auto name = [=](int layer) {
      return multi ? "inception_s" + std::to_string(S - 1) + "_l_" + std::to_string(layer) : "inception" + std::to_string(layer);
    };
    build_ss_tower(g.experts[0], 0, S, name, "", 3, /*last_relu=*/false, multi ? 4 : 5);
  }

  // ms_sw_n_est.get_model (models/ms_sw_n_est.py:41-89): noise_est_net on the LARGE scale (scale 1) with a ReLU on
  // its single output (:172), normal_est_net 'small' on scale 0 and 'large' on scale 1 (:77-78); the driver keeps
  // n_est_small where noise_est < 0.015 (:80-82).  Here: gate = the noise tower, expert 0 = small, expert 1 = large.
  void build_switch() {
    auto scoped = [](const std::string& sfx) {
      return [sfx](int layer) { return "inception" + std::to_string(layer) + sfx; };
    };
    build_ss_tower(g.gate, 1, 1, scoped("noise"), "noise", 1, /*last_relu=*/true, 5);
    build_ss_tower(g.experts[0], 0, 1, scoped("small"), "small", 3, /*last_relu=*/false, 5);
    build_ss_tower(g.experts[1], 1, 1, scoped("large"), "large", 3, /*last_relu=*/false, 5);
  }

  // normal_est_net, 8^3 branch (models/experts_n_est.py:243-291)
  void build_expert(int i) {
    Tower& T = g.experts[i];
    init_tower(T);
    const int lo = g.cfg.expert_scale_lo[i], cnt = g.cfg.expert_scale_cnt[i];
    ChanMap m; m.C = g.mups_cstride;
    for (int c = 0; c < 20 * cnt; ++c) m.pos.push_back(20 * lo + c);   // MuPS[..., start:end]  :100-102
    const std::string s = "Expert_" + std::to_string(i);
    if (g.cfg.grid_n == 3) {   // models/experts_n_est.py:275-276: the 3^3 branch ignores `divider`
      ChanMap flat;
      const int pb = conv_net_3g(T, s + "_expert_conv", m, &flat);
      T.out_buf = fc_stack(T, pb, flat, {"fc1" + s, "fc2" + s, "fc3" + s, "fc4" + s}, {512, 128, 64, 3}, /*last_relu=*/false, flat.C);
      T.n_out = 3;
      return;
    }
    const int F1 = 128 / cnt;   // np.round(128 / divider) under Python-2 integer division  :254
    x8 = g.x8; x8_block = 0;
    int b = inception(T, "inception1" + s, 0, m, F1, 3, 5, 3, &m);
    b = inception(T, "inception2" + s, b, m, 256, 3, 5, 3, &m, true);    // + maxpool3  :261
    x8 = false;
    b = inception(T, "inception4" + s, b, m, 256, 2, 4, 2, &m, true);    // + maxpool5  :266
    b = inception(T, "inception6" + s, b, m, 512, 2, 4, 1, &m, true);    // + maxpool7  :271
    T.out_buf = fc_stack(T, b, m, {"fc1" + s, "fc2" + s, "fc3" + s, "fc4" + s}, {512, 128, 64, 3}, /*last_relu=*/false);
    T.n_out = 3;
  }
};

}  // namespace

int build_graph(const nesti_config_t* cfg, Graph* g, bool x8) {
  if (cfg->arch != NESTI_ARCH_EXPERTS && cfg->arch != NESTI_ARCH_SINGLE && cfg->arch != NESTI_ARCH_MULTI &&
      cfg->arch != NESTI_ARCH_SWITCH)
    NESTI_FAIL("unknown arch");
  if (cfg->arch == NESTI_ARCH_SWITCH && cfg->n_scales != 2)
    NESTI_FAIL("NESTI_ARCH_SWITCH (ms_sw_n_est) takes exactly two scales (models/ms_sw_n_est.py:50)");
  if (cfg->arch == NESTI_ARCH_SINGLE && cfg->n_scales != 1) NESTI_FAIL("NESTI_ARCH_SINGLE (ss_norm_est) takes exactly one scale");
  if (cfg->grid_n != 8 && !(cfg->grid_n == 3 && cfg->arch == NESTI_ARCH_EXPERTS))
    NESTI_FAIL("the Gaussian grid must be 8^3 (any model) or 3^3 (experts_n_est only: the ablation models are 8^3-only, "
               "models/ms_sw_n_est.py:183)");
  if (cfg->n_scales < 1 || cfg->n_scales > NESTI_MAX_SCALES) NESTI_FAIL("bad n_scales");
  if (cfg->n_experts < 1 || cfg->n_experts > NESTI_MAX_EXPERTS) NESTI_FAIL("bad n_experts");
  for (int i = 0; i < cfg->n_experts && cfg->arch == NESTI_ARCH_EXPERTS; ++i) {
    if (cfg->expert_scale_cnt[i] < 1 || cfg->expert_scale_lo[i] < 0 ||
        cfg->expert_scale_lo[i] + cfg->expert_scale_cnt[i] > cfg->n_scales)
      NESTI_FAIL("expert scale range outside [0, n_scales)");
  }
  g->cfg = *cfg;
  g->x8 = x8 && cfg->arch == NESTI_ARCH_EXPERTS && cfg->grid_n == 8;
  g->mups_cstride = pad_to(20 * cfg->n_scales, kPad);
  g->layers.clear();
  Builder b(*g);
  g->gate = Tower();
  g->gate2 = Tower();
  if (cfg->arch == NESTI_ARCH_SINGLE || cfg->arch == NESTI_ARCH_MULTI) {
    g->cfg.n_experts = 1;
    g->experts.assign(1, Tower());
    b.build_single();
    return 0;
  }
  if (cfg->arch == NESTI_ARCH_SWITCH) {
    g->cfg.n_experts = 2;
    g->cfg.expert_scale_lo[0] = 0; g->cfg.expert_scale_lo[1] = 1;
    g->cfg.expert_scale_cnt[0] = g->cfg.expert_scale_cnt[1] = 1;
    g->experts.assign(2, Tower());
    b.build_switch();
    return 0;
  }
  b.build_gate();
  if (g->x8) b.build_gate2();
  g->experts.assign(cfg->n_experts, Tower());
  for (int i = 0; i < cfg->n_experts; ++i) b.build_expert(i);
  return 0;
}

}  // namespace nesti
