// C ABI of libxvec_hip.so, the batch planner: xv_plan_create turns (node, frame offsets) into the list of steps xv_forward
// runs (api_forward.hip).  It is a short driver over phases that each take their inputs as arguments and return a value:
// (a) shape, (b) order, (c) fusion decisions, (d) one step at a time -- GEMM form, scratch, output placement --, (e) two-unit
// chaining, (f) output info, (g) device index arrays.  Only (g) calls HIP.  tests/test_gpu_plan_golden.py pins the result.
#include "xv_arena.h"
#include "xv_model.h"

using namespace xv;
using namespace xv::api;

namespace {

// Plan index arrays come from / go back to a per-handle pool: a ragged ark stream creates one plan per batch, and
// hipMalloc / hipFree (device-synchronising) per batch would serialise the host with the GPU.
constexpr size_t kPoolMaxBuffers = 96, kPoolMaxBytes = (size_t)1 << 30;

hipError_t pool_take(xv_handle* h, size_t bytes, DevBuf& out) {
  out = DevBuf();
  if (bytes == 0) return hipSuccess;
  {
    std::lock_guard<std::mutex> lk(h->pool_mu);
    int best = -1;
    for (size_t i = 0; i < h->pool.size(); ++i)
      if (h->pool[i].bytes >= bytes && h->pool[i].bytes <= 4 * bytes + 4096 &&
          (best < 0 || h->pool[i].bytes < h->pool[best].bytes))
        best = (int)i;
    if (best >= 0) {
      out = h->pool[best];
      h->pool_bytes -= out.bytes;
      h->pool.erase(h->pool.begin() + best);
      return hipSuccess;
    }
  }
  const size_t cap = (bytes + 4095) / 4096 * 4096;
  const hipError_t e = hipMalloc(&out.p, cap);
  if (e == hipSuccess) out.bytes = cap; else out = DevBuf();
  return e;
}

void pool_give(xv_handle* h, DevBuf& b) {
  if (!b.p) return;
  {
    std::lock_guard<std::mutex> lk(h->pool_mu);
    if (h->pool.size() < kPoolMaxBuffers && h->pool_bytes + b.bytes <= kPoolMaxBytes) {
      h->pool.push_back(b);
      h->pool_bytes += b.bytes;
      b = DevBuf();
      return;
    }
  }
  b.release();
}

// ------------------------------------------------------------------------------ (a) shape
struct BatchShape {
  int B = 0;
  bool uniform = true;              // every utterance has the same length
  int max_level = 0;
  std::vector<int32_t> lvl[4];      // frame offsets per time level (tf 'same' with stride 2: ceil(L / 2) frames; model/resnet.py:187)
  int64_t Fl[4] = {0, 0, 0, 0};     // total frames of the batch per time level
};

int plan_shape(xv_handle* h, const int32_t* frame_offsets, int batch, int node_id, BatchShape* out) {
  if (frame_offsets[0] != 0) return fail(h, XV_ERR_INVALID, "frame_offsets[0] must be 0");
  const int need_ctx = xv_node_context(h, node_id);
  BatchShape& sh = *out;
  sh.B = batch;
  for (int b = 0; b < batch; ++b) {
    const int64_t len = (int64_t)frame_offsets[b + 1] - frame_offsets[b];
    if (len <= need_ctx)
      return fail(h, XV_ERR_TOO_SHORT, "utterance %d has %lld frames; node '%s' needs more than %d", b, (long long)len,
                  h->nodes[node_id].name.c_str(), need_ctx);
    if (len != (int64_t)frame_offsets[1] - frame_offsets[0]) sh.uniform = false;
  }
  const int64_t F0 = frame_offsets[batch];
  if (F0 > (int64_t)1 << 30) return fail(h, XV_ERR_INVALID, "batch of %lld frames is too large for 32-bit row indices", (long long)F0);
  for (const Value& v : h->values) sh.max_level = std::max(sh.max_level, v.tlevel);
  for (int64_t& f : sh.Fl) f = F0;
  sh.lvl[0].assign(frame_offsets, frame_offsets + batch + 1);
  for (int k = 1; k <= sh.max_level && k < 4; ++k) {
    sh.lvl[k].resize(batch + 1);
    sh.lvl[k][0] = 0;
    for (int b = 0; b < batch; ++b) sh.lvl[k][b + 1] = sh.lvl[k][b] + (sh.lvl[k - 1][b + 1] - sh.lvl[k - 1][b] + 1) / 2;
    sh.Fl[k] = sh.lvl[k][batch];
  }
  return XV_OK;
}

// ------------------------------------------------------------------------------ (b) order
std::vector<int> producers(const xv_handle* h) {       // value id -> producing op (-1: the network input)
  std::vector<int> producer(h->values.size(), -1);
  for (size_t i = 0; i < h->ops.size(); ++i) producer[h->ops[i].out] = (int)i;
  return producer;
}

// ops needed for the node (backward closure), in topological (= creation) order
std::vector<int> plan_order(const xv_handle* h, int target_op, const std::vector<int>& producer) {
  std::vector<char> need(h->ops.size(), 0);
  std::vector<int> stack{target_op};
  while (!stack.empty()) {
    const int o = stack.back();
    stack.pop_back();
    if (need[o]) continue;
    need[o] = 1;
    for (int in : {h->ops[o].in0, h->ops[o].in1})
      if (in > 0 && producer[in] >= 0) stack.push_back(producer[in]);
  }
  std::vector<int> order;
  for (size_t i = 0; i < h->ops.size(); ++i) if (need[i]) order.push_back((int)i);
  return order;
}

// ------------------------------------------------------------------------------ (c) fusion decisions
struct Fusion {
  int key_prod = -1;            // op of the last key layer when it emits score partials instead of the key
  int val_prod = -1;            // op of the value layer when it emits weighted moments instead of the value
  int att_pool_value = -1;      // ... and that value
  int fused_value = -1;         // value whose statistics pooling runs in its producer's epilogue
  int slot_value = -1;          // the value whose rows are pooled per 64-row slot (fused_value or att_pool_value)
  std::vector<int> order;       // the steps' ops; a fused value layer is moved behind the softmax
  std::vector<int32_t> slotbase;   // [B] slot base per utterance of slot_value
  int64_t pool_slots = 0;
};

int readers_of(const xv_handle* h, const std::vector<int>& order, int v) {
  int n = 0;
  for (int o : order)
    if (h->ops[o].in0 == v || h->ops[o].in1 == v) ++n;
  return n;
}

// the op that produces v, if its epilogue can take an attention fusion (one-tap split layer, v read once); else -1
int att_fusable(const xv_handle* h, const std::vector<int>& order, const std::vector<int>& producer, int target_op, int v) {
  if (v <= 0 || producer[v] < 0 || producer[v] == target_op) return -1;
  const Op& prod = h->ops[producer[v]];
  if (prod.kind != OP_GEMM || prod.in1 > 0 || readers_of(h, order, v) != 1) return -1;
  const Layer& L = h->layers[prod.layer];
  return (L.use_split && !L.im2col && L.mode == 0 && L.w == 1 && (L.cout & 3) == 0) ? producer[v] : -1;
}

Fusion plan_fusion(const xv_handle* h, int target_op, const std::vector<int>& producer, std::vector<int> order, const BatchShape& sh) {
  Fusion f;
  // Fused attentive pooling (bf16x3 kernel, attention epilogue): the last key layer emits score partials instead of
  // the key when the scores are its only reader; the value layer emits weighted moments instead of the value when
  // the pooling is its only reader -- it then has to run AFTER the softmax, so it is moved behind it in the order.
  if (h->opt_att_fusion && h->desc.pooling_type == XV_POOL_SELF_ATTENTION && h->desc.att_num_heads <= 8) {
    int softmax_op = -1, pool_op = -1;
    for (int o : order) {
      if (h->ops[o].kind == OP_ATT_SCORES) f.key_prod = att_fusable(h, order, producer, target_op, h->ops[o].in0);
      if (h->ops[o].kind == OP_ATT_SOFTMAX) softmax_op = o;
      if (h->ops[o].kind == OP_ATT_POOL) pool_op = o;
    }
    if (pool_op >= 0 && softmax_op >= 0) {
      const int H = h->desc.att_num_heads, dv = h->att_dv;
      const bool heads_ok = H == 1 || !h->desc.att_split_value || (dv / H) % 32 == 0;
      const int vp = heads_ok ? att_fusable(h, order, producer, target_op, h->ops[pool_op].in0) : -1;
      if (vp >= 0) {
        f.val_prod = vp;
        f.att_pool_value = h->ops[pool_op].in0;
        order.erase(std::find(order.begin(), order.end(), vp));
        order.insert(std::find(order.begin(), order.end(), pool_op), vp);
      }
    }
  }
  // statistics pooling fused into the epilogue of the dense layer that feeds it, when that
  // layer's output has no other reader in this plan
  for (int o : order) {
    const Op& op = h->ops[o];
    if (op.kind != OP_STAT_POOL || op.in0 <= 0 || producer[op.in0] < 0) continue;
    const Op& prod = h->ops[producer[op.in0]];
    if (prod.kind != OP_GEMM || producer[op.in0] == target_op) continue;
    const Layer& L = h->layers[prod.layer];
    if (readers_of(h, order, op.in0) == 1 && L.w == 1 && (L.cout & 3) == 0 && h->opt_pool_fusion) f.fused_value = op.in0;
  }
  f.slot_value = f.fused_value >= 0 ? f.fused_value : f.att_pool_value;
  if (f.slot_value >= 0) {
    const int ctx = h->values[f.slot_value].ctx;
    const std::vector<int32_t>& so = sh.lvl[h->values[f.slot_value].tlevel];
    f.slotbase.resize(sh.B);
    for (int b = 0; b < sh.B; ++b) {
      const int r0 = so[b] - b * ctx, r1 = so[b + 1] - (b + 1) * ctx;
      const int t0 = r0 >> 6, t1 = (r1 - 1) >> 6;
      f.slotbase[b] = (int32_t)(f.pool_slots - t0);
      f.pool_slots += t1 - t0 + 1;
    }
  }
  f.order = std::move(order);
  return f;
}

// ------------------------------------------------------------------------------ (d) one step
struct PlanCtx {                    // what phases (a) - (c) decided: read-only from here on
  const xv_handle* h;
  const Node& node;
  const BatchShape& sh;
  const Fusion& fu;
  int64_t rows(int v) const { return value_rows(h, v, sh.Fl, sh.B); }
};

struct RowMaps {                    // element offsets of the steps' row maps in one device array
  std::vector<int64_t> off;
  int64_t elems = 0;
  int add(int64_t n) { off.push_back(elems); elems += n; return (int)off.size() - 1; }
};

struct Placement {                  // where the values live in the workspace while the steps are laid out
  Arena arena;
  std::vector<int64_t> off, size, off_sb, size_sb;      // fp32 / split-blocked copy per value (size 0: not owned)
  std::vector<char> want_f32, want_sb;                  // which copies have a reader
  std::vector<int> last_use;                            // last step index that reads each value
  void free_value(int v) {
    if (size[v] > 0) { arena.release(off[v], size[v]); size[v] = 0; }
    if (size_sb[v] > 0) { arena.release(off_sb[v], size_sb[v]); size_sb[v] = 0; }
  }
};

// liveness, and which formats of each value are read: fp32 by the f32 GEMM / pooling / elementwise kernels,
// split-blocked by the bf16x3 GEMM
Placement make_placement(const xv_handle* h, const std::vector<int>& order) {
  const size_t nv = h->values.size();
  Placement pl;
  pl.off.assign(nv, -1); pl.off_sb.assign(nv, -1);
  pl.size.assign(nv, 0); pl.size_sb.assign(nv, 0);
  pl.want_f32.assign(nv, 0); pl.want_sb.assign(nv, 0);
  pl.last_use.assign(nv, -1);
  for (size_t s = 0; s < order.size(); ++s) {
    const Op& op = h->ops[order[s]];
    const bool split_in = op.kind == OP_GEMM && h->layers[op.layer].use_split;
    if (op.in0 > 0) (split_in ? pl.want_sb : pl.want_f32)[op.in0] = 1;
    if (op.in1 > 0) pl.want_f32[op.in1] = 1;
    for (int in : {op.in0, op.in1})
      if (in > 0) pl.last_use[in] = (int)s;
  }
  return pl;
}

// GEMM rows of one layer: their form and number, whether they cover the output's border, and the row-map slots
void gemm_form(const PlanCtx& c, const Op& op, const Layer& L, PlanStep& st, RowMaps& rm) {
  const xv_handle* h = c.h;
  const int64_t padded_rows = c.sh.Fl[st.lvl_in] + 2 * (int64_t)c.sh.B;   // input time rows incl. the two border rows per utterance
  const bool grid = L.mode == 1 || L.mode == 2;
  if (L.mode == 0) {
    st.form = FORM_ROWS;
    st.M = (int)(st.rows_in - (L.w - 1));
  } else if (L.mode == 1 && L.use_f6) {   // rows = padded time rows, frequency bins = a second tile dimension (csrc/grid.hip)
    st.form = FORM_TROWS;
    st.M = (int)padded_rows;
  } else if (grid && L.use_split && h->opt_grid_compact && st.rows_in * (int64_t)sb_ld(L.cin) * 4 < ((int64_t)1 << 32)) {
    st.form = FORM_COMPACT;               // rows = output bins; 32-bit byte offsets of the window positions
    st.M = (int)(c.sh.Fl[st.lvl_out] * L.Fout);
  } else if (grid) {
    st.form = FORM_GRID;
    st.M = (int)(padded_rows * (h->values[op.in0].grid_S / L.sw));
  } else if (L.mode == 3) {
    st.form = FORM_CONV5;
    st.M = (int)padded_rows;
  } else {                                // conv0: one row per output grid position
    st.form = FORM_CONV0;
    st.M = (int)(padded_rows * h->values[op.out].grid_S);
  }
  // does every border position of the output get a zero-writing GEMM row? (csrc/grid.hip)  If not the value is
  // zeroed as a whole before the layer runs.
  if (st.form == FORM_GRID) st.grid_cover = L.st == 1 && h->values[op.in0].grid_S / L.sw == h->values[op.out].grid_S;
  else st.grid_cover = st.form == FORM_CONV0;
  if (L.w > 1 || L.mode != 0) {
    st.rowmap = rm.add(align_up(st.M, 64));
    if (st.compact()) st.arow = rm.add(align_up(st.M, 128));
  }
  const int64_t valid_out = L.mode == 0 ? st.rows_out : c.sh.Fl[st.lvl_out] * (L.mode == 3 ? 1 : L.Fout);
  st.flops = 2 * valid_out * (int64_t)L.cout * L.K();
  st.bytes = 4 * (st.rows_in * L.cin + st.rows_out * L.cout + (int64_t)L.K() * L.cout);
}

// Per-step scratch of a GEMM (staged input rows, split-K partials; K-split tail plan), taken from the arena.  The caller
// releases {scratch, scratch2} bytes once the step's outputs are placed.
std::pair<int64_t, int64_t> gemm_scratch(const PlanCtx& c, const Op& op, const Layer& L, PlanStep& st, Arena& arena) {
  const xv_handle* h = c.h;
  const bool fused = op.out == c.fu.fused_value || st.op == c.fu.key_prod || st.op == c.fu.val_prod;
  int64_t scratch = 0, held = 0, held2 = 0;
  if (L.mode == 4) {
    scratch = ((int64_t)st.M + kSlackRows) * 32 * 4;              // conv0 im2col rows (K = 9 padded to 32)
  } else if (L.im2col) {
    scratch = L.cin_pad ? (st.rows_in + kSlackRows) * (int64_t)L.cin_pad * 4 : (st.M + kSlackRows) * (int64_t)L.Kpad * 4;
  } else if (!L.use_split && op.out != c.fu.fused_value) {
    st.ksplit = gemm_f32_ksplit(st.M, L.Kpad, L.Npad);
    if (st.ksplit > 1) scratch = (int64_t)st.ksplit * st.M * L.Npad * 4;
  } else if (L.use_f6) {
    scratch = (st.rows_in + kSlackRows) * (int64_t)sb_ld(L.cin) * 4;      // the input in the block format of gemm_f16f6.hip
    if (h->opt_tail_split && op.in1 <= 0 && L.mode == 0) {
      const int64_t part = gemm_bf16x3_tail_plan(st.M, L.Kpad, L.Npad, L.w, &st.tail_mt, &st.ksplit, 4);
      if (part > 0) {
        held2 = align_up(part, kAlign);
        st.scratch2_off = arena.alloc(held2);
      }
    }
  } else if (L.use_split && L.mode == 0 && !fused && op.in1 <= 0 && h->opt_tail_split) {
    scratch = gemm_bf16x3_tail_plan(st.M, L.Kpad, L.Npad, L.w, &st.tail_mt, &st.ksplit);
  }
  if (scratch > 0) {
    held = align_up(scratch, kAlign);
    st.scratch_off = arena.alloc(held);
  }
  return {held, held2};
}

// traffic / work estimate of the ops that are not layers (profiler, dominant step), and their fused forms
void op_cost(const PlanCtx& c, const Op& op, PlanStep& st) {
  const xv_handle* h = c.h;
  const int64_t slots = c.fu.pool_slots;
  const int heads = h->desc.att_num_heads;
  const int64_t cols_in = op.in0 >= 0 ? h->values[op.in0].cols : 0, cols_out = h->values[op.out].cols;
  if (op.kind == OP_AFFINE_ACT) {
    st.stage = st.to_out ? c.node.stage : 2;
    st.bytes = 8 * st.rows_out * cols_out;
  } else if (op.kind == OP_ATT_POOL && c.fu.val_prod >= 0) {      // finalize only: reads the weighted (s1, m2) slots
    st.fuse_att = 1;
    st.bytes = 4 * (slots * (2 * (h->pool_dim / 2) + heads) + st.rows_out * cols_out);
    st.flops = 8 * slots * (h->pool_dim / 2);
  } else if (op.kind == OP_STAT_POOL || op.kind == OP_ATT_POOL) {
    st.bytes = 4 * (st.rows_in * cols_in + st.rows_out * cols_out);
    st.flops = 4 * st.rows_in * cols_in;
    if (op.kind == OP_STAT_POOL && op.in0 == c.fu.fused_value) {      // finalize only: reads the (sum, M2) slots
      st.fuse_pool = true;
      st.bytes = 4 * (slots * 2 * cols_in + st.rows_out * cols_out);
      st.flops = 6 * slots * cols_in;
    }
  } else if (op.kind == OP_ATT_SCORES) {
    st.bytes = 4 * st.rows_in * cols_in;
    st.flops = 2 * st.rows_in * (int64_t)h->att_dk_h * heads;
    if (c.fu.key_prod >= 0) {           // reduce form: reads the partial planes
      st.fuse_att = 1;
      st.att_ld = align_up(st.rows_in, 64);
      st.bytes = 4 * (st.att_ld * (h->key_npad / 32) + st.rows_in) * heads;
    }
  } else {
    st.bytes = 8 * st.rows_out * cols_out;
  }
}

const PlanStep* softmax_step(const xv_handle* h, const std::vector<PlanStep>& done) {
  const PlanStep* found = nullptr;
  for (const PlanStep& prev : done)
    if (h->ops[prev.op].kind == OP_ATT_SOFTMAX) found = &prev;
  return found;
}

// Where the step's output goes.  The softmax works in place on the scores buffer; the requested node writes the caller's
// buffer (a grid-valued one through a padded copy); everything else gets its own block(s) in the arena.
void place_output(const PlanCtx& c, const Op& op, PlanStep& st, const std::vector<PlanStep>& done, Placement& pl) {
  const xv_handle* h = c.h;
  const int heads = h->desc.att_num_heads;
  const int v = op.out;
  auto take = [&](int64_t bytes) {         // an fp32-side block for the output
    pl.size[v] = bytes;
    pl.off[v] = pl.arena.alloc(bytes);
    st.out_off = pl.off[v];
  };
  if (op.kind == OP_ATT_SOFTMAX) {
    pl.off[v] = pl.off[op.in0];
    pl.size[v] = pl.size[op.in0];
    pl.size[op.in0] = 0;                   // ownership moves to the softmax value
    st.out_off = pl.off[v];
    if (c.fu.val_prod >= 0) {              // the per-slot weight sums live behind the weights (block sized by ATT_SCORES)
      st.fuse_att = 1;
      st.att_s0_off = pl.off[v] + align_up(st.rows_out * (int64_t)heads * 4, kAlign);
    }
    return;
  }
  if (st.to_out && !c.node.att_weights) {
    if (h->values[v].grid_F == 0) {
      st.out_off = -1;                     // straight into the caller's output buffer (fp32)
    } else {
      st.unpad_to_out = true;              // grid-valued node: padded grid in the workspace, then unpad into `out`
      take(value_bytes(h, v, c.sh.Fl, c.sh.B));
    }
    return;
  }
  if (op.kind == OP_GEMM && st.op == c.fu.key_prod) {
    const Layer& L = h->layers[op.layer];
    st.fuse_att = 1;                       // [Npad / 32][H] planes of partial scores, row stride att_ld
    st.att_ld = align_up(st.rows_out, 64);
    take(align_up((int64_t)(L.Npad / 32) * heads * st.att_ld * 4, kAlign));
    st.bytes = 4 * (st.rows_in * L.cin + (int64_t)L.K() * L.cout) + pl.size[v];
  } else if (op.kind == OP_GEMM && st.op == c.fu.val_prod) {
    const Layer& L = h->layers[op.layer];
    st.fuse_att = 2;                       // weighted (s1, m2) per slot and output column
    take(align_up(c.fu.pool_slots * 2 * (int64_t)(h->pool_dim / 2) * 4, kAlign));
    st.bytes = 4 * (st.rows_in * L.cin + (int64_t)L.K() * L.cout + st.rows_out * heads) + pl.size[v];
    if (const PlanStep* sm = softmax_step(h, done)) { st.att_w_off = sm->out_off; st.att_s0_off = sm->att_s0_off; }
  } else if (v == c.fu.fused_value) {
    st.fuse_pool = true;
    take(align_up(c.fu.pool_slots * 2 * (int64_t)h->values[v].cols * 4, kAlign));
  } else if (pl.want_f32[v] || c.node.att_weights) {
    if (op.kind == OP_ATT_SCORES && c.fu.val_prod >= 0)       // + the per-slot weight sums written by the softmax step
      take(align_up(st.rows_out * (int64_t)heads * 4, kAlign) + align_up(c.fu.pool_slots * (int64_t)heads * 4, kAlign) + kAlign);
    else
      take(value_bytes(h, v, c.sh.Fl, c.sh.B));
  }
  if (pl.want_sb[v]) {
    pl.size_sb[v] = value_sb_bytes(h, v, c.sh.Fl, c.sh.B);
    pl.off_sb[v] = pl.arena.alloc(pl.size_sb[v]);
    st.out_sb_off = pl.off_sb[v];
  }
}

// The PlanStep of op order[s]: geometry, kernel form, scratch and output; then its scratch and the inputs it read last
// go back to the arena.
PlanStep plan_step(const PlanCtx& c, size_t s, const std::vector<PlanStep>& done, Placement& pl, RowMaps& rm) {
  const xv_handle* h = c.h;
  const Op& op = h->ops[c.fu.order[s]];
  PlanStep st;
  st.op = c.fu.order[s];
  st.to_out = st.op == c.node.op;
  st.rows_in = op.in0 >= 0 ? c.rows(op.in0) : 0;
  st.rows_out = c.rows(op.out);
  st.lvl_in = op.in0 >= 0 ? h->values[op.in0].tlevel : 0;
  st.lvl_out = h->values[op.out].tlevel;
  st.frames_out = c.sh.Fl[st.lvl_out];
  st.in0_off = op.in0 == 0 ? -2 : (op.in0 > 0 ? pl.off[op.in0] : -1);
  st.in0_sb_off = op.in0 > 0 ? pl.off_sb[op.in0] : -1;
  st.in1_off = op.in1 > 0 ? pl.off[op.in1] : -1;
  std::pair<int64_t, int64_t> scratch{0, 0};
  if (op.kind == OP_GEMM) {
    const Layer& L = h->layers[op.layer];
    st.stage = st.to_out ? c.node.stage : L.final_stage();
    gemm_form(c, op, L, st, rm);
    scratch = gemm_scratch(c, op, L, st, pl.arena);
  } else {
    op_cost(c, op, st);
  }
  place_output(c, op, st, done, pl);
  if (op.kind == OP_ATT_POOL && c.fu.val_prod >= 0)
    if (const PlanStep* sm = softmax_step(h, done)) st.att_s0_off = sm->att_s0_off;
  if (scratch.first > 0) pl.arena.release(st.scratch_off, scratch.first);
  if (scratch.second > 0) pl.arena.release(st.scratch2_off, scratch.second);
  for (int in : {op.in0, op.in1})
    if (in > 0 && pl.last_use[in] == (int)s) pl.free_value(in);
  return st;
}

// ------------------------------------------------------------------------------ (e) two-unit chaining
// two-unit layers back to back: the producer's epilogue writes the consumer's block format directly when nobody else reads
// the value (no fp32 copy, not the requested node, final stage) -- otherwise the consumer converts the split-blocked rows
void chain_two_unit(const xv_handle* h, std::vector<PlanStep>& steps) {
  for (PlanStep& cs : steps) {
    const Op& cop = h->ops[cs.op];
    if (cop.kind != OP_GEMM || !h->layers[cop.layer].use_f6) continue;
    const bool grid = h->layers[cop.layer].mode == 1;
    // readers of the value's SPLIT copy: every op that takes it as its first input; a second input is the fp32 residual of a ResNet
    // block (another copy of the value) -- in the TDNN graphs it does not occur, and disqualifies as before
    // Several readers are fine when every one of them is a two-unit layer.
    if (cs.in_f6) continue;                // (marked with an earlier reader of the same value)
    int readers = 0;
    bool all_f6 = true;
    PlanStep* prod = nullptr;
    for (PlanStep& os : steps) {
      const Op& o = h->ops[os.op];
      if (o.in0 == cop.in0 || (!grid && o.in1 == cop.in0)) {
        ++readers;
        if (o.kind != OP_GEMM || !h->layers[o.layer].use_f6 || o.in0 != cop.in0) all_f6 = false;
      }
      if (o.out == cop.in0) prod = &os;
    }
    if (!prod || !all_f6 || (grid && readers != 1)) continue;
    const Op& pop = h->ops[prod->op];
    if (pop.kind != OP_GEMM) continue;
    const Layer& PL = h->layers[pop.layer];
    if (prod->to_out || prod->out_sb_off < 0 || prod->stage != PL.final_stage()) continue;
    if (grid) {
      // producers: another two-unit grid layer (its residual epilogue also writes the fp32 copy and adds a residual), or a stride-2
      // 3 x 3 convolution of the gathered f16 kernel (EPI = 3: the block format only)
      const bool gather = PL.mode == 1 && !PL.use_f6 && PL.use_split && prod->compact() && prod->out_off < 0 && pop.in1 <= 0;
      if (!((PL.mode == 1 && PL.use_f6) || gather)) continue;
    } else {
      // producers that can write the format: another two-unit layer, or a layer of the f16 kernels with one tap (the dense layers
      // between the convolutions of the extended TDNN) or >= 5 taps -- their EPI = 3 forms; a K-split tail of theirs is finished by the
      // two-unit kernel's reduce (launch_f6v2_tail_reduce)
      const bool f16_layer = PL.mode == 0 && PL.use_split && !PL.use_f6 && (PL.w == 1 ? !PL.im2col : PL.w >= 5 && PL.w <= 9) &&
                             (PL.im2col ? PL.cin_pad > 0 : PL.cin % 32 == 0) && prod->fuse_att == 0 && !prod->fuse_pool;
      if (!((PL.mode == 0 && PL.use_f6) || f16_layer) || prod->out_off >= 0 || pop.in1 > 0) continue;
    }
    prod->out_f6 = true;
    for (PlanStep& os : steps) {
      const Op& o = h->ops[os.op];
      if (o.kind == OP_GEMM && o.in0 == cop.in0 && h->layers[o.layer].use_f6) os.in_f6 = true;
    }
    // a one-tap producer keeps the three-slab kernel for all its tiles: its K-split tail (raw slices of the two-slab kernel + the
    // block-format reduce) costs more than the third of a round it saves (extended TDNN in-process A/B: 2.192 -> 2.172 ms,
    // profiles/r03/ab_onetap_f6_notail.txt)
    if (!grid && PL.mode == 0 && !PL.use_f6 && PL.w == 1) { prod->tail_mt = 0; prod->ksplit = 1; }
  }
}

// ------------------------------------------------------------------------------ (f) output info
xv_plan_info plan_output_info(const xv_handle* h, int node_id, const BatchShape& sh, int64_t flops, int64_t arena_top) {
  const Node& node = h->nodes[node_id];
  const int out_value = h->ops[node.op].out;
  const Value& vout = h->values[out_value];
  xv_plan_info I{};
  I.struct_size = (int32_t)sizeof(xv_plan_info);
  I.node_id = node_id;
  I.batch = sh.B;
  I.in_frames = sh.Fl[0];
  I.flops = flops;
  if (node.att_weights) {                 // [b, h, l]: equal lengths (checked by the driver)
    I.frame_level = 0;
    I.out_rows = (int64_t)sh.B * h->desc.att_num_heads;
    I.out_cols = (sh.lvl[0][1] - sh.lvl[0][0]) - vout.ctx;
  } else if (vout.grid_F > 0) {
    I.frame_level = 1;
    I.out_rows = sh.Fl[vout.tlevel] * vout.grid_F;       // [sum L_b, F, C] without the border
    I.out_cols = vout.cols;
  } else {
    I.frame_level = vout.frame_level ? 1 : 0;
    I.out_rows = value_rows(h, out_value, sh.Fl, sh.B);
    I.out_cols = vout.cols;
  }
  I.workspace_bytes = align_up(arena_top, kAlign) + kAlign;
  return I;
}

// ------------------------------------------------------------------------------ (g) device index arrays
// the row map of one GEMM step, by the form the planner recorded for it
hipError_t build_rowmap(const xv_plan* p, const PlanStep& st, hipStream_t s) {
  const xv_handle* h = p->h;
  const Op& op = h->ops[st.op];
  const Layer& L = h->layers[op.layer];
  const int B = p->info.batch;
  const Value& vi = h->values[op.in0];
  const Value& vo = h->values[op.out];
  const int32_t* doff = p->dev_offsets(st.lvl_in);
  int32_t* maps = static_cast<int32_t*>(p->d_rowmaps.p);
  int32_t* rm = maps + p->rowmap_off[st.rowmap];
  switch (st.form) {
    case FORM_ROWS: return launch_build_rowmap(doff, B, vi.ctx, L.w, rm, st.M, s);
    case FORM_TROWS: return launch_build_rowmap_trows(doff, B, vo.grid_S, rm, st.M, s);
    case FORM_COMPACT:
      return launch_build_rowmap_grid_compact(doff, p->dev_offsets(st.lvl_out), B, vi.grid_S, vo.grid_S, L.Fout, L.sw, L.st,
                                              L.mode == 1 ? 3 : 1, maps + p->rowmap_off[st.arow], rm, st.M, align_up(st.M, 128), s);
    case FORM_GRID:
      if (L.st == 2)
        return launch_build_rowmap_grid_ts(doff, p->dev_offsets(st.lvl_out), B, vi.grid_S / L.sw, L.Fout, vo.grid_S,
                                           L.mode == 1 ? 3 : 1, rm, st.M, s);
      return launch_build_rowmap_grid(doff, B, vi.grid_S / L.sw, L.Fout, vo.grid_S, st.grid_cover ? 1 : 0, rm, st.M, s);
    case FORM_CONV5: return launch_build_rowmap_rows(doff, B, rm, st.M, s);
    default: return launch_build_rowmap_interior(doff, B, L.Fout, vo.grid_S, rm, st.M, s);
  }
}

// Offsets, level offsets, row maps, row2utt and slot bases: filled in stream order, ahead of any xv_forward enqueued on
// `s` afterwards, without host synchronisation (the host copies they are filled from belong to the plan).
hipError_t upload_index_arrays(xv_plan* p, const BatchShape& sh, int64_t rowmap_elems, int slot_value, hipStream_t s, const char** what) {
  xv_handle* h = p->h;
  const size_t nb = (size_t)(sh.B + 1) * 4;
  hipError_t e = hipSuccess;
  DeviceGuard g(h->device);
  *what = "hipMalloc(offsets)";
  if ((e = pool_take(h, nb, p->d_offsets)) != hipSuccess) return e;
  *what = "hipMemcpyAsync(offsets)";
  if ((e = hipMemcpyAsync(p->d_offsets.p, p->lvl_offsets[0].data(), nb, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  for (int k = 1; k <= sh.max_level && k < 4; ++k) {
    *what = "hipMalloc(level offsets)";
    if ((e = pool_take(h, nb, p->d_lvl[k])) != hipSuccess) return e;
    *what = "hipMemcpyAsync(level offsets)";
    if ((e = hipMemcpyAsync(p->d_lvl[k].p, p->lvl_offsets[k].data(), nb, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  }
  if (rowmap_elems > 0) {
    *what = "hipMalloc(rowmaps)";
    if ((e = pool_take(h, (size_t)rowmap_elems * 4, p->d_rowmaps)) != hipSuccess) return e;
    *what = "build_rowmap";
    for (const PlanStep& st : p->steps)
      if (st.rowmap >= 0 && (e = build_rowmap(p, st, s)) != hipSuccess) return e;
  }
  if (slot_value >= 0) {
    const int64_t rows = value_rows(h, slot_value, sh.Fl, sh.B);
    *what = "hipMalloc(row2utt)";
    if ((e = pool_take(h, (size_t)rows * 4, p->d_row2utt)) != hipSuccess) return e;
    *what = "hipMalloc(slotbase)";
    if ((e = pool_take(h, (size_t)sh.B * 4, p->d_slotbase)) != hipSuccess) return e;
    *what = "hipMemcpyAsync(slotbase)";
    if ((e = hipMemcpyAsync(p->d_slotbase.p, p->offsets_slotbase.data(), (size_t)sh.B * 4, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    *what = "build_row2utt";
    e = launch_build_row2utt(p->dev_offsets(h->values[slot_value].tlevel), sh.B, h->values[slot_value].ctx,
                             static_cast<int32_t*>(p->d_row2utt.p), (int)rows, s);
  }
  return e;
}

}  // namespace

extern "C" {

int xv_plan_create(xv_handle* h, const int32_t* frame_offsets, int batch, int node_id, void* stream, xv_plan** out) {
  if (!h) return fail(nullptr, XV_ERR_INVALID, "xv_plan_create: null handle");
  if (!out || !frame_offsets) return fail(h, XV_ERR_INVALID, "xv_plan_create: null argument");
  *out = nullptr;
  if (!h->finalized) return fail(h, XV_ERR_STATE, "xv_plan_create before xv_finalize");
  if (batch < 1) return fail(h, XV_ERR_INVALID, "xv_plan_create: batch %d < 1", batch);
  if (node_id < 0 || node_id >= (int)h->nodes.size()) return fail(h, XV_ERR_INVALID, "xv_plan_create: bad node id %d", node_id);
  const Node& node = h->nodes[node_id];
  BatchShape sh;
  if (const int rc = plan_shape(h, frame_offsets, batch, node_id, &sh)) return rc;
  if (node.att_weights && !sh.uniform)
    return fail(h, XV_ERR_INVALID, "attention_weights [b,h,l] needs utterances of equal length");
  const std::vector<int> producer = producers(h);
  const Fusion fu = plan_fusion(h, node.op, producer, plan_order(h, node.op, producer), sh);

  xv_plan* p = new (std::nothrow) xv_plan();
  if (!p) return fail(h, XV_ERR_HIP, "out of host memory");
  p->h = h;
  for (int k = 0; k <= sh.max_level && k < 4; ++k) p->lvl_offsets[k] = sh.lvl[k];
  p->pool_slots = fu.pool_slots;
  p->offsets_slotbase = fu.slotbase;

  const PlanCtx ctx{h, node, sh, fu};
  Placement pl = make_placement(h, fu.order);
  RowMaps rm;
  int64_t total_flops = 0;
  for (size_t s = 0; s < fu.order.size(); ++s) {
    p->steps.push_back(plan_step(ctx, s, p->steps, pl, rm));
    total_flops += p->steps.back().flops;
  }
  p->rowmap_off = rm.off;
  for (size_t i = 0; i < p->steps.size(); ++i)
    if (p->steps[i].flops > p->steps[p->dominant_step].flops) p->dominant_step = (int)i;
  chain_two_unit(h, p->steps);
  p->info = plan_output_info(h, node_id, sh, total_flops, pl.arena.top());

  const char* what = "";
  const hipError_t e = upload_index_arrays(p, sh, rm.elems, fu.slot_value, static_cast<hipStream_t>(stream), &what);
  if (e != hipSuccess) {
    const int rc = fail(h, XV_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    xv_plan_destroy(p);
    return rc;
  }
  *out = p;
  return XV_OK;
}

int xv_plan_query(const xv_plan* p, xv_plan_info* info) {
  if (!p || !info) return XV_ERR_INVALID;
  *info = p->info;
  return XV_OK;
}

void xv_plan_destroy(xv_plan* p) {
  if (!p) return;
  {
    DeviceGuard g(p->h->device);
    pool_give(p->h, p->d_offsets);
    for (int k = 1; k < 4; ++k) pool_give(p->h, p->d_lvl[k]);
    pool_give(p->h, p->d_rowmaps);
    pool_give(p->h, p->d_row2utt);
    pool_give(p->h, p->d_slotbase);
  }
  delete p;
}

}  // extern "C"
