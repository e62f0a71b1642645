// C ABI of libxvec_hip.so (include/xvec_hip.h), the model graph: xv_create builds the predict graph of the reference
// (model/tdnn.py:36-181, model/resnet.py:152-351, model/pooling.py:8-240, model/trainer.py:385-405) as layers, ops, values
// and nodes; tensors, options, node queries and xv_destroy.  The weights are packed in api_weights.hip.
#include <cstdarg>

#include "xv_model.h"

using namespace xv;
using namespace xv::api;

namespace xv {
namespace api {

thread_local std::string g_last_error;  // failures with no handle (xv_create)

int fail(xv_handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) {
    std::lock_guard<std::mutex> lk(h->err_mu);
    h->err = buf;
  }
  g_last_error = buf;
  return code;
}

}  // namespace api
}  // namespace xv

namespace {

void expect(xv_handle* h, const std::string& name, std::vector<int64_t> shape) {
  HostTensor t;
  t.shape = std::move(shape);
  h->tensors[name] = std::move(t);
}

void expect_bn(xv_handle* h, const std::string& scope, int n) {
  for (const char* s : {"gamma", "beta", "moving_mean", "moving_variance"}) expect(h, scope + "/" + s, {n});
}

// adds layer + op + value + nodes; returns the output value id
int add_layer(xv_handle* h, const std::string& var_scope, const std::string& ep_prefix, bool conv, int w,
              int cin, int cout, bool has_bn, int act, int in_value, bool frame_level, int ctx_out,
              int kernel_rank = 4) {
  Layer L;
  const std::string kind = conv ? "_conv" : "_dense";
  L.kernel_name = var_scope + kind + "/kernel";
  L.bias_name = var_scope + kind + "/bias";
  L.w = w; L.cin = cin; L.cout = cout; L.has_bn = has_bn; L.act = act;
  if (conv && kernel_rank == 4) expect(h, L.kernel_name, {1, w, cin, cout});      // tf.layers.conv2d (1,w): HWIO
  else if (conv) expect(h, L.kernel_name, {w, cin, cout});                         // tf.layers.conv1d
  else expect(h, L.kernel_name, {cin, cout});
  expect(h, L.bias_name, {cout});
  L.ep[ST_AFFINE] = ep_prefix + kind;
  if (has_bn) {
    L.bn_scope = var_scope + "_bn";
    expect_bn(h, L.bn_scope, cout);
    L.ep[ST_BN] = ep_prefix + "_bn";
  }
  if (act != ACT_NONE) {
    L.ep[ST_ACT] = ep_prefix + (act == ACT_TANH ? "_tanh" : "_relu");
    if (act == ACT_PRELU) {
      L.alpha_name = var_scope + "_relu/alpha";
      expect(h, L.alpha_name, {cout});
    }
  }
  const int li = (int)h->layers.size();
  h->layers.push_back(std::move(L));
  Value v; v.frame_level = frame_level; v.ctx = ctx_out; v.cols = cout;
  const int vid = (int)h->values.size();
  h->values.push_back(v);
  Op op; op.kind = OP_GEMM; op.layer = li; op.in0 = in_value; op.out = vid;
  const int oi = (int)h->ops.size();
  h->ops.push_back(op);
  for (int s = 0; s < 3; ++s) {
    const std::string& e = h->layers[li].ep[s];
    if (!e.empty()) { Node n; n.name = e; n.op = oi; n.stage = s; h->nodes.push_back(n); }
  }
  return vid;
}

int add_simple_op(xv_handle* h, int kind, int in0, int in1, bool frame_level, int ctx, int cols) {
  Value v; v.frame_level = frame_level; v.ctx = ctx; v.cols = cols;
  const int vid = (int)h->values.size();
  h->values.push_back(v);
  Op op; op.kind = kind; op.in0 = in0; op.in1 = in1; op.out = vid;
  h->ops.push_back(op);
  return vid;
}

void add_node(xv_handle* h, const std::string& name, int op, int stage, bool attw = false) {
  Node n; n.name = name; n.op = op; n.stage = stage; n.att_weights = attw;
  h->nodes.push_back(n);
}

// one ResNet convolution (+BN, + optional activation / residual); returns the output value id
int add_conv2d(xv_handle* h, const std::string& var, const std::string& bn, const std::string& relu, int mode, int cin,
               int cout, int Fin, int Fout, int sw, int act, int in_value, int residual_value, const char* node_name,
               int st = 1) {
  Layer L;
  L.mode = mode; L.cin = cin; L.cout = cout; L.Fin = Fin; L.Fout = Fout; L.sw = sw; L.w = 1; L.st = st;
  L.kernel_name = var + "/kernel";
  L.has_bias = (mode == 3);
  if (mode == 1 || mode == 4) expect(h, L.kernel_name, {3, 3, cin, cout});
  else if (mode == 2) expect(h, L.kernel_name, {1, 1, cin, cout});
  else expect(h, L.kernel_name, {1, Fin, cin, cout});
  if (L.has_bias) { L.bias_name = var + "/bias"; expect(h, L.bias_name, {cout}); }
  L.has_bn = true;
  L.bn_scope = bn;
  expect_bn(h, bn, cout);
  L.act = act;
  if (act == ACT_PRELU) { L.alpha_name = relu + "/alpha"; expect(h, L.alpha_name, {cout}); }
  L.ep[act != ACT_NONE ? ST_ACT : ST_BN] = node_name ? node_name : "";
  const int li = (int)h->layers.size();
  h->layers.push_back(std::move(L));
  Value v; v.cols = cout;
  v.tlevel = h->values[in_value].tlevel + (st == 2 ? 1 : 0);
  if (mode == 3) { v.frame_level = true; v.ctx = 0; } else { v.grid_F = Fout; }
  const int vid = (int)h->values.size();
  h->values.push_back(v);
  Op op; op.kind = OP_GEMM; op.layer = li; op.in0 = in_value; op.in1 = residual_value; op.out = vid;
  h->ops.push_back(op);
  if (node_name) add_node(h, node_name, (int)h->ops.size() - 1, act != ACT_NONE ? ST_ACT : ST_BN);
  return vid;
}

// model/resnet.py:152-351 (resnet_18): conv0, four stages of [conv_block, identity_block...], conv5,
// dense1, dense2, pooling, tdnn6, tdnn7.  `channels` = width of stage 1 (64 in the reference).
// Block outputs are exposed as extra nodes (conv0_relu, conv1a, ..., conv5_relu, dense*_relu) for
// tests only, and so are the two inner values of a residual block: "<block>_relu0", the first convolution behind its
// activation, and "<block>_short", the projection shortcut behind its normalisation (`a` blocks only); the reference
// registers just pooling / tdnn6_* / tdnn7_* / output.
int build_resnet(xv_handle* h) {
  const xv_model_desc& d = h->desc;
  const int act = act_of(d);
  const std::string sc = "resnet_18/";
  if (d.feat_dim != 40) return fail(h, XV_ERR_INVALID, "resnet_18 needs 40-dim features (model/resnet.py:190)");
  if (d.pooling_type != XV_POOL_STATISTICS)
    return fail(h, XV_ERR_UNSUPPORTED, "resnet_18 registers no frame-level endpoints: only statistics_pooling is possible");
  h->values.clear();
  Value in; in.frame_level = true; in.ctx = 0; in.cols = 40;
  h->values.push_back(in);
  int F = 40, cin = d.channels;
  int v = add_conv2d(h, sc + "conv0_1", sc + "conv0_bn", sc + "conv0_relu", 4, 1, cin, F, F, 1, act, 0, -1, "conv0_relu");
  if (d.resnet_maxpooling) {                       // model/resnet.py:230-231
    Value pv; pv.grid_F = F; pv.cols = cin;
    const int vid = (int)h->values.size();
    h->values.push_back(pv);
    Op op; op.kind = OP_GRID_MAXPOOL; op.in0 = v; op.out = vid;
    h->ops.push_back(op);
    add_node(h, "conv0_max", (int)h->ops.size() - 1, -1);
    v = vid;
  }
  for (int stage = 1; stage <= 4; ++stage) {
    const int nf = d.channels << (stage - 1);
    const int sw = stage == 1 ? 1 : 2;
    const int Fo = F / sw;
    for (int bi = 0; bi < d.resnet_blocks[stage - 1]; ++bi) {
      char nm[32];
      if (bi == 0) snprintf(nm, sizeof(nm), "conv%da", stage); else snprintf(nm, sizeof(nm), "conv%db_%d", stage, bi - 1);
      const std::string b = sc + nm;
      const int s_w = bi == 0 ? sw : 1, Fi = bi == 0 ? F : Fo;
      const int s_t = (bi == 0 && stage > 1 && d.resnet_time_stride) ? 2 : 1;       // model/resnet.py:187,239,244,249
      const std::string n_relu0 = std::string(nm) + "_relu0", n_short = std::string(nm) + "_short";
      const int c0 = add_conv2d(h, b + "_conv0", b + "_bn0", b + "_relu0", 1, cin, nf, Fi, Fo, s_w, act, v, -1, n_relu0.c_str(), s_t);
      int shortcut = v;
      if (bi == 0)      // projection shortcut: 1x1 conv + BN (model/resnet.py:71-83)
        shortcut = add_conv2d(h, b + "_conv_short", b + "_bn_short", "", 2, cin, nf, Fi, Fo, s_w, ACT_NONE, v, -1, n_short.c_str(), s_t);
      v = add_conv2d(h, b + "_conv1", b + "_bn1", b + "_relu_final", 1, nf, nf, Fo, Fo, 1, act, c0, shortcut, nm);
      cin = nf;
    }
    F = Fo;
  }
  v = add_conv2d(h, sc + "conv5", sc + "conv5_bn", sc + "conv5_relu", 3, cin, cin, F, 1, 1, act, v, -1, "conv5_relu");
  h->final_ctx = 0;
  // dense1 / dense2 (model/resnet.py:270-290): variables "<name>/kernel", BN "<name>_bn", PReLU "<name>_relu/alpha"
  auto dense_named = [&](const char* name, int ci, int co, int in_v) {
    Layer L;
    L.kernel_name = sc + name + "/kernel"; L.bias_name = sc + name + "/bias";
    L.w = 1; L.cin = ci; L.cout = co; L.has_bn = true; L.act = act;
    expect(h, L.kernel_name, {ci, co}); expect(h, L.bias_name, {co});
    L.bn_scope = sc + name + "_bn"; expect_bn(h, L.bn_scope, co);
    if (act == ACT_PRELU) { L.alpha_name = sc + name + "_relu/alpha"; expect(h, L.alpha_name, {co}); }
    L.ep[ST_ACT] = std::string(name) + "_relu";
    const int li = (int)h->layers.size();
    h->layers.push_back(std::move(L));
    Value vv; vv.frame_level = true; vv.ctx = 0; vv.cols = co; vv.tlevel = h->values[in_v].tlevel;
    const int vid = (int)h->values.size();
    h->values.push_back(vv);
    Op op; op.kind = OP_GEMM; op.layer = li; op.in0 = in_v; op.out = vid;
    h->ops.push_back(op);
    add_node(h, std::string(name) + "_relu", (int)h->ops.size() - 1, ST_ACT);
    return vid;
  };
  v = dense_named("dense1", cin, cin, v);
  v = dense_named("dense2", cin, d.num_nodes_pooling_layer, v);
  h->pool_dim = 2 * d.num_nodes_pooling_layer;
  const int pooled = add_simple_op(h, OP_STAT_POOL, v, -1, false, 0, h->pool_dim);
  add_node(h, "pooling", (int)h->ops.size() - 1, -1);
  v = add_layer(h, sc + "tdnn6", "tdnn6", false, 1, h->pool_dim, cin, true, act, pooled, false, 0);
  v = add_layer(h, sc + "tdnn7", "tdnn7", false, 1, cin, d.num_nodes_last_layer, !d.last_layer_no_bn,
                d.last_layer_linear ? ACT_NONE : act, v, false, 0);
  if (d.feature_norm) {
    add_simple_op(h, OP_L2_SCALE, v, -1, false, 0, d.num_nodes_last_layer);
    add_node(h, "output", (int)h->ops.size() - 1, -1);
  } else {
    const int last = (int)h->ops.size() - 1;
    add_node(h, "output", last, h->layers[h->ops[last].layer].final_stage());
  }
  // Pitch of the grid values, one per stage (= per number of frequency bins, so that a layer's input, output and
  // residual share it): F + 1 (shared border column) unless a value of the stage is read at frequency stride 2, which
  // needs an even pitch -> F + 2.  With the default blocks: 42, 22, 12 for stages 1-3 and 6 for stage 4.
  std::vector<int> wide;
  for (const Op& op : h->ops) {
    if (op.kind != OP_GEMM) continue;
    const Layer& L = h->layers[op.layer];
    if ((L.mode == 1 || L.mode == 2) && L.sw == 2 && op.in0 > 0) wide.push_back(h->values[op.in0].grid_F);
  }
  for (Value& v : h->values)
    if (v.grid_F > 0) v.grid_S = v.grid_F + (std::find(wide.begin(), wide.end(), v.grid_F) != wide.end() ? 2 : 1);
  return XV_OK;
}

// Build the predict graph for `desc`: model/tdnn.py:36-181 (tdnn) or :343-591 (etdnn).
int build_graph(xv_handle* h) {
  const xv_model_desc& d = h->desc;
  if (d.network_type == XV_NET_RESNET18) return build_resnet(h);
  const int C = d.channels, act = act_of(d);
  h->values.clear();
  Value in; in.frame_level = true; in.ctx = 0; in.cols = d.feat_dim;
  h->values.push_back(in);   // value 0 = network input
  // frame-level layer table: kernel width per layer (1 = dense); the last one feeds the pooling
  static const int kTdnn[] = {5, 5, 7, 1, 1};
  static const int kEtdnn[] = {5, 1, 5, 1, 7, 1, 9, 1, 1, 1};
  const bool et = d.network_type == XV_NET_ETDNN;
  const int* widths = et ? kEtdnn : kTdnn;
  const int nframe = et ? 10 : 5;
  const std::string scope = et ? "etdnn/" : "tdnn/";
  std::vector<int> frame_value(nframe + 1, -1);   // value id of layer i's output (1-based)
  int v = 0, ctx = 0, cin = d.feat_dim;
  for (int i = 1; i <= nframe; ++i) {
    const int w = widths[i - 1];
    ctx += w - 1;
    const int cout = (i == nframe) ? d.num_nodes_pooling_layer : C;
    char nm[16];
    snprintf(nm, sizeof(nm), "tdnn%d", i);
    v = add_layer(h, scope + nm, nm, w > 1, w, cin, cout, true, act, v, true, ctx, et ? 3 : 4);
    frame_value[i] = v;
    cin = cout;
  }
  h->final_ctx = ctx;
  const int v_last = v;

  int pooled;
  if (d.pooling_type == XV_POOL_STATISTICS) {
    h->pool_dim = 2 * d.num_nodes_pooling_layer;
    pooled = add_simple_op(h, OP_STAT_POOL, v_last, -1, false, 0, h->pool_dim);
    add_node(h, "pooling", (int)h->ops.size() - 1, -1);
  } else if (d.pooling_type == XV_POOL_SELF_ATTENTION) {
    auto pick = [&](int which) {     // a frame layer whose output already has the full temporal context
      if (which < 1 || which > nframe) return -1;
      return h->values[frame_value[which]].ctx == ctx ? frame_value[which] : -1;
    };
    int key = pick(d.att_key_input), val = pick(d.att_value_input);
    if (key < 0 || val < 0)
      return fail(h, XV_ERR_UNSUPPORTED, "att_key_input/att_value_input must be a tdnn<N>_relu at full temporal context");
    if (d.att_num_key_layers < 1 || d.att_num_key_layers > XV_MAX_ATT_LAYERS || d.att_num_value_layers < 0 ||
        d.att_num_value_layers > XV_MAX_ATT_LAYERS)
      return fail(h, XV_ERR_INVALID, "attention: bad number of key/value layers");
    auto kind_to = [&](int kind, bool& bn, int& a) {
      bn = kind == 2;
      a = (kind == 1 || kind == 2) ? act : (kind == 3 ? ACT_TANH : ACT_NONE);
    };
    const std::string base = scope + "attention/";
    for (int i = 0; i < d.att_num_key_layers; ++i) {                       // model/pooling.py:100-116
      bool bn; int a;
      kind_to(i < d.att_num_key_layers - 1 ? 2 : d.att_key_network_type, bn, a);
      char nm[32]; snprintf(nm, sizeof(nm), "att_key%d", i);
      key = add_layer(h, base + nm + "/" + nm, nm, false, 1, h->values[key].cols, d.att_key_num_nodes[i], bn, a, key, true, ctx);
    }
    for (int i = 0; i < d.att_num_value_layers; ++i) {                     // model/pooling.py:119-135
      bool bn; int a;
      kind_to(i < d.att_num_value_layers - 1 ? 2 : d.att_value_network_type, bn, a);
      char nm[32]; snprintf(nm, sizeof(nm), "att_value%d", i);
      val = add_layer(h, base + nm + "/" + nm, nm, false, 1, h->values[val].cols, d.att_value_num_nodes[i], bn, a, val, true, ctx);
    }
    const int H = d.att_num_heads;
    h->att_dk = h->values[key].cols;
    h->att_dv = h->values[val].cols;
    if (H < 1) return fail(h, XV_ERR_INVALID, "att_num_heads must be >= 1");
    if (d.att_split_key && h->att_dk % H) return fail(h, XV_ERR_INVALID, "key dim %d not divisible by %d heads", h->att_dk, H);
    if (d.att_split_value && h->att_dv % H) return fail(h, XV_ERR_INVALID, "value dim %d not divisible by %d heads", h->att_dv, H);
    h->att_dk_h = d.att_split_key ? h->att_dk / H : h->att_dk;
    expect(h, scope + "attention/query", {H, h->att_dk_h});
    const int sc = add_simple_op(h, OP_ATT_SCORES, key, -1, true, ctx, H);
    const int sm = add_simple_op(h, OP_ATT_SOFTMAX, sc, -1, true, ctx, H);
    add_node(h, "attention_weights", (int)h->ops.size() - 1, -1, true);
    h->pool_dim = 2 * (d.att_split_value ? h->att_dv : h->att_dv * H);
    pooled = add_simple_op(h, OP_ATT_POOL, val, sm, false, 0, h->pool_dim);
    add_node(h, "att_output_before_nonlinear", (int)h->ops.size() - 1, -1);
    if (d.att_apply_nonlinear) {                                           // model/pooling.py:222-229
      h->post_bn_scope = scope + "attention/att_post_bn";
      expect_bn(h, h->post_bn_scope, h->pool_dim);
      if (act == ACT_PRELU) {
        h->post_alpha_name = scope + "attention/att_post_relu/alpha";
        expect(h, h->post_alpha_name, {h->pool_dim});
      }
      pooled = add_simple_op(h, OP_AFFINE_ACT, pooled, -1, false, 0, h->pool_dim);
      add_node(h, "att_post_bn", (int)h->ops.size() - 1, 1);
      add_node(h, "att_post_relu", (int)h->ops.size() - 1, 2);
    }
    add_node(h, "pooling", (int)h->ops.size() - 1, d.att_apply_nonlinear ? 2 : -1);
  } else {
    return fail(h, XV_ERR_UNSUPPORTED, "Not implement pooling_type %d", d.pooling_type);
  }
  // segment-level layers: tdnn6/tdnn7 (model/tdnn.py:137-179) or tdnn12/tdnn13 (:547-589)
  char s1[16], s2[16];
  snprintf(s1, sizeof(s1), "tdnn%d", et ? 12 : 6);
  snprintf(s2, sizeof(s2), "tdnn%d", et ? 13 : 7);
  v = add_layer(h, scope + s1, s1, false, 1, h->pool_dim, C, true, act, pooled, false, 0);
  v = add_layer(h, scope + s2, s2, false, 1, C, d.num_nodes_last_layer, !d.last_layer_no_bn,
                d.last_layer_linear ? ACT_NONE : act, v, false, 0);
  if (d.feature_norm) {                                                     // model/trainer.py:400-403
    add_simple_op(h, OP_L2_SCALE, v, -1, false, 0, d.num_nodes_last_layer);
    add_node(h, "output", (int)h->ops.size() - 1, -1);
  } else {
    const int last = (int)h->ops.size() - 1;
    add_node(h, "output", last, h->layers[h->ops[last].layer].final_stage());
  }
  return XV_OK;
}

}  // namespace

// ============================================================================ C ABI
extern "C" {

const char* xv_version(void) { return "xvec_hip 0.1 gfx950"; }

const char* xv_last_error(const xv_handle* h) { return h ? h->err.c_str() : g_last_error.c_str(); }

int xv_create(const xv_model_desc* desc, int device, xv_handle** out) {
  if (!desc || !out) return fail(nullptr, XV_ERR_INVALID, "xv_create: null argument");
  *out = nullptr;
  if (desc->struct_size != (int32_t)sizeof(xv_model_desc))
    return fail(nullptr, XV_ERR_INVALID, "xv_create: xv_model_desc size %d != %zu (ABI mismatch)", desc->struct_size,
                sizeof(xv_model_desc));
  if (desc->network_type != XV_NET_TDNN && desc->network_type != XV_NET_ETDNN && desc->network_type != XV_NET_RESNET18)
    return fail(nullptr, XV_ERR_UNSUPPORTED, "Not implement network_type %d (tdnn, extended_tdnn, resnet_18)", desc->network_type);
  if (desc->network_type == XV_NET_RESNET18)
    for (int i = 0; i < 4; ++i)
      if (desc->resnet_blocks[i] < 1 || desc->resnet_blocks[i] > 16)
        return fail(nullptr, XV_ERR_INVALID, "xv_create: resnet_blocks[%d] = %d", i, desc->resnet_blocks[i]);
  if (desc->feat_dim < 1 || desc->channels < 1 || desc->num_nodes_pooling_layer < 1 || desc->num_nodes_last_layer < 1)
    return fail(nullptr, XV_ERR_INVALID, "xv_create: non-positive layer width");
  if (desc->precision != XV_PREC_F32 && desc->precision != XV_PREC_BF16X3 && desc->precision != XV_PREC_F16X3 &&
      desc->precision != XV_PREC_F16F6)
    return fail(nullptr, XV_ERR_INVALID, "xv_create: unknown precision %d", desc->precision);
  if (desc->relu_type < XV_ACT_RELU || desc->relu_type > XV_ACT_PRELU)
    return fail(nullptr, XV_ERR_INVALID, "xv_create: unknown relu_type %d", desc->relu_type);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(nullptr, XV_ERR_HIP, "xv_create: HIP device %d not available (%d visible)", device, ndev);
  xv_handle* h = new (std::nothrow) xv_handle();
  if (!h) return fail(nullptr, XV_ERR_HIP, "xv_create: out of host memory");
  h->desc = *desc;
  h->device = device;
  const int rc = build_graph(h);
  if (rc != XV_OK) {
    g_last_error = h->err;
    delete h;
    return rc;
  }
  *out = h;
  return XV_OK;
}

int xv_set_tensor(xv_handle* h, const char* tf_name, const float* host, const int64_t* shape, int rank) {
  if (!h) return fail(nullptr, XV_ERR_INVALID, "xv_set_tensor: null handle");
  if (!tf_name || !host || !shape || rank < 1) return fail(h, XV_ERR_INVALID, "xv_set_tensor: null argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->finalized) return fail(h, XV_ERR_STATE, "xv_set_tensor after xv_finalize");
  auto it = h->tensors.find(tf_name);
  if (it == h->tensors.end()) return fail(h, XV_ERR_INVALID, "variable '%s' is not part of the predict graph", tf_name);
  HostTensor& t = it->second;
  bool same = (int)t.shape.size() == rank;
  int64_t n = 1;
  for (int i = 0; i < rank; ++i) {
    if (same && t.shape[i] != shape[i]) same = false;
    n *= shape[i];
  }
  if (!same) {
    std::string exp, got;
    for (auto s : t.shape) exp += std::to_string(s) + ",";
    for (int i = 0; i < rank; ++i) got += std::to_string(shape[i]) + ",";
    return fail(h, XV_ERR_INVALID, "variable '%s': expected shape [%s] got [%s]", tf_name, exp.c_str(), got.c_str());
  }
  t.data.assign(host, host + n);
  t.set = true;
  return XV_OK;
}

int xv_set_option(xv_handle* h, const char* name, int value) {
  if (!h || !name) return fail(h, XV_ERR_INVALID, "xv_set_option: null argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!strcmp(name, "pool_fusion")) h->opt_pool_fusion = value != 0;
  else if (!strcmp(name, "tail_split")) h->opt_tail_split = value != 0;
  else if (!strcmp(name, "att_fusion")) h->opt_att_fusion = value != 0;
  else if (!strcmp(name, "slab3")) h->opt_slab3 = value != 0;
  else if (!strcmp(name, "first_walk")) h->opt_first_walk = value < 0 ? 0 : (value > 2 ? 2 : value);
  else if (!strcmp(name, "grid_f6")) h->opt_grid_f6 = value != 0;      // (before xv_finalize: it decides the weight formats)
  else if (!strcmp(name, "grid_compact")) h->opt_grid_compact = value != 0;
  else if (!strcmp(name, "profile_dominant")) h->opt_profile_dominant = value != 0;
  else return fail(h, XV_ERR_INVALID, "xv_set_option: unknown option '%s'", name);
  return XV_OK;
}

int xv_node_id(const xv_handle* h, const char* name) {
  if (!h || !name) return XV_ERR_INVALID;
  for (size_t i = 0; i < h->nodes.size(); ++i)
    if (h->nodes[i].name == name) return (int)i;
  return XV_ERR_INVALID;
}

int xv_node_context(const xv_handle* h, int node_id) {
  if (!h || node_id < 0 || node_id >= (int)h->nodes.size()) return XV_ERR_INVALID;
  const Op& op = h->ops[h->nodes[node_id].op];
  const Value& v = h->values[op.out];
  return v.frame_level ? v.ctx : h->final_ctx;
}

int xv_layer_two_unit(const xv_handle* h, const char* endpoint_name) {
  if (!h || !endpoint_name) return XV_ERR_INVALID;
  if (!h->finalized) return XV_ERR_STATE;
  for (const Node& n : h->nodes)
    if (n.name == endpoint_name) {
      const Op& op = h->ops[n.op];
      if (op.kind != OP_GEMM) return XV_ERR_INVALID;
      return h->layers[op.layer].use_f6 ? 1 : 0;
    }
  return XV_ERR_INVALID;
}

void xv_destroy(xv_handle* h) {
  if (!h) return;
  {
    DeviceGuard g(h->device);
    for (auto& L : h->layers) { L.wt.release(); L.wsb.release(); L.wfr.release(); L.vec.release(); L.wf6m.release(); L.wf6x.release(); L.wdir.release(); }
    h->query.release();
    h->ovf_flag.release();
    h->query_eff.release();
    h->post_vec.release();
    for (auto& b : h->pool) b.release();
    for (auto e : h->prof_pool) (void)hipEventDestroy(e);
  }
  delete h;
}

}  // extern "C"
