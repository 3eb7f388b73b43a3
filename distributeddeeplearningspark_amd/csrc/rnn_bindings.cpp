// pybind11 registrations of the persistent GRU / LSTM / SimpleRNN kernels (kernels/rnn.hip).
// The input projection, the input gradient and (off the fused path) the parameter-gradient
// contractions run on the fp32 MFMA GEMM (kernels/gemm_f32.hip); no library GEMM is called.
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <ATen/DeviceGuard.h>

#include "ddl_ops.h"

namespace py = pybind11;
using namespace ddl;

namespace {

inline hipStream_t cur_stream() { return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }

int cell_id(const std::string& cell) {
  TORCH_CHECK(cell == "gru" || cell == "lstm" || cell == "rnn", "rnn: cell must be 'gru', 'lstm' or 'rnn'");
  return cell == "gru" ? 0 : (cell == "lstm" ? 1 : 2);
}
int gates_of(int c) { return c == 0 ? 3 : (c == 1 ? 4 : 1); }

// C[M][N] (fp32, row-major ldc) = alpha * A B + beta * C with element strides (gemm_f32)
void f32mm(const at::Tensor& a, long sam, long sak, const at::Tensor& b, long sbk, long sbn, at::Tensor& c, long ldc,
           int64_t M, int64_t N, int64_t K, float beta = 0.f, const float* bias = nullptr) {
  const int e = gemm_f32(a.data_ptr<float>(), sam, sak, b.data_ptr<float>(), sbk, sbn, c.data_ptr<float>(), ldc, (int)M,
                         (int)N, (int)K, 1.f, beta, bias, 0, cur_stream());
  TORCH_CHECK(e == 0, "gemm_f32 launch failed: ", hipGetErrorString((hipError_t)e));
}

// ------------------------------------------------------------------------------------------------
// Directed recurrences (go_backwards / Bidirectional; RnnDir in ddl_ops.h): ndir = 1 or 2 directions over the
// same x in ONE recurrence launch per pass.  merge: 0 none (one direction), 1 concat, 2 sum, 3 ave.
// Saved tensors are stacked over the direction: hs / cs [ndir][B][T+1][H], gates [ndir][B][T][GH].
struct DirWeights {
  at::Tensor W, U, b;  // b undefined: no bias
};

std::vector<DirWeights> dir_weights(const py::list& Ws, const py::list& Us, const py::list& bs, int64_t I, int64_t G) {
  const size_t nd = Ws.size();
  TORCH_CHECK((nd == 1 || nd == 2) && Us.size() == nd && bs.size() == nd, "rnn: one or two directions");
  std::vector<DirWeights> out(nd);
  for (size_t d = 0; d < nd; ++d) {
    out[d].W = Ws[d].cast<at::Tensor>().contiguous();
    out[d].U = Us[d].cast<at::Tensor>().contiguous();
    if (!bs[d].is_none()) out[d].b = bs[d].cast<at::Tensor>().contiguous();
    const int64_t H = out[0].U.size(0);
    for (const at::Tensor* t : {&out[d].W, &out[d].U})
      TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat, "rnn: fp32 GPU weights");
    TORCH_CHECK(out[d].W.size(0) == I && out[d].W.size(1) == G * H && out[d].U.size(0) == H && out[d].U.size(1) == G * H,
                "rnn: W [I,GH], U [H,GH] (equal shapes in both directions)");
    TORCH_CHECK(!out[d].b.defined() || (out[d].b.scalar_type() == at::kFloat && out[d].b.numel() == G * H),
                "rnn: bias [GH] fp32");
    TORCH_CHECK(out[d].b.defined() == out[0].b.defined(), "rnn: both directions with or without bias");
  }
  return out;
}

int merge_id(const std::string& m) {
  TORCH_CHECK(m == "concat" || m == "sum" || m == "ave", "birnn: merge_mode must be 'concat', 'sum' or 'ave'");
  return m == "concat" ? 1 : (m == "sum" ? 2 : 3);
}

// the step mask of x [B,T,..] as the kernels read it (null when there is none)
const unsigned char* mask_ptr(const c10::optional<at::Tensor>& mask, const at::Tensor& x, const char* who) {
  if (!mask) return nullptr;
  TORCH_CHECK(mask->scalar_type() == at::kByte && mask->dim() == 2 && mask->size(0) == x.size(0) &&
                  mask->size(1) == x.size(1), who, ": mask must be uint8 [B, T]");
  TORCH_CHECK(mask->is_contiguous() && mask->device() == x.device(), who,
              ": mask must be contiguous and on the input's device");
  return mask->data_ptr<unsigned char>();
}

// Dropout masks of a directed call (ddl_ops.h): per direction the input multipliers dp [G, B, I] and the recurrent
// ones rdp [G, B, H], each kind given for every direction or for none.
struct DropSet {
  std::vector<at::Tensor> dp, rdp;  // empty: none
  bool any() const { return !dp.empty() || !rdp.empty(); }
};

std::vector<at::Tensor> drop_list(const std::vector<c10::optional<at::Tensor>>& ms, const at::Tensor& x, int64_t G,
                                  int64_t n, size_t nd, const char* who, const char* what) {
  size_t given = 0;
  for (const auto& m : ms) given += m.has_value();
  if (!given) return {};
  TORCH_CHECK(ms.size() == nd && given == nd, who, ": ", what, " for every direction or for none");
  std::vector<at::Tensor> out;
  for (const auto& m : ms) {
    TORCH_CHECK(m->scalar_type() == at::kFloat && m->dim() == 3 && m->size(0) == G && m->size(1) == x.size(0) &&
                    m->size(2) == n, who, ": ", what, " must be fp32 [G, B, ", n, "]");
    TORCH_CHECK(m->is_contiguous() && m->device() == x.device(), who, ": ", what,
                " must be contiguous and on the input's device");
    out.push_back(*m);
  }
  return out;
}

DropSet drop_set(const std::vector<c10::optional<at::Tensor>>& dps, const std::vector<c10::optional<at::Tensor>>& rdps,
                 const at::Tensor& x, int64_t G, int64_t H, size_t nd, const char* who) {
  TORCH_CHECK(x.dim() == 3, who, ": x [B,T,I] fp32 on GPU");
  return {drop_list(dps, x, G, x.size(2), nd, who, "dropout_mask"),
          drop_list(rdps, x, G, H, nd, who, "recurrent_dropout_mask")};
}

py::tuple dir_fwd(int c, const at::Tensor& x, const std::vector<DirWeights>& w, const std::vector<int>& rev, bool rs,
                  int merge, bool yproc, int64_t act, int64_t ract, const c10::optional<at::Tensor>& mask,
                  const DropSet& drop = {}) {
  const int G = gates_of(c);
  const int nd = (int)w.size();
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 3, "rnn_fwd: x [B,T,I] fp32 on GPU");
  const int64_t B = x.size(0), T = x.size(1), I = x.size(2), H = w[0].U.size(0);
  TORCH_CHECK(T >= 1, "rnn_fwd: empty sequence");
  const unsigned char* mk = mask_ptr(mask, x, "rnn_fwd");
  at::DeviceGuard g(x.device());
  at::Tensor xc = x.contiguous();
  auto opt = x.options();
  at::Tensor xw;
  const bool reg = rnn_reg_path(c, (int)H, (int)act, (int)ract);
  if (!drop.dp.empty()) {
    // input dropout: gate g's column block of xw projects its own masked copy of x, all T steps at once
    xw = at::empty({nd, B * T, G * H}, opt);
    at::Tensor xm = at::empty({G, B * T, I}, opt);
    for (int d = 0; d < nd; ++d) {
      int e = rnn_drop_x(xc.data_ptr<float>(), drop.dp[d].data_ptr<float>(), xm.data_ptr<float>(), G, (int)B, (int)T,
                         (int)I, cur_stream());
      TORCH_CHECK(e == 0, "rnn_drop_x launch failed: ", hipGetErrorString((hipError_t)e));
      for (int g = 0; g < G; ++g) {
        e = gemm_f32(xm.data_ptr<float>() + g * B * T * I, I, 1, w[d].W.data_ptr<float>() + g * H, G * H, 1,
                     xw.data_ptr<float>() + d * B * T * G * H + g * H, G * H, (int)(B * T), (int)H, (int)I, 1.f, 0.f,
                     w[d].b.defined() ? w[d].b.data_ptr<float>() + g * H : nullptr, 0, cur_stream());
        TORCH_CHECK(e == 0, "gemm_f32 launch failed: ", hipGetErrorString((hipError_t)e));
      }
    }
  } else if (!(reg && rnn_fuses_input((int)H, (int)I)) || drop.any()) {  // one projection GEMM per direction
    xw = at::empty({nd, B * T, G * H}, opt);                             // (recurrent dropout: never fused)
    for (int d = 0; d < nd; ++d) {
      at::Tensor xwd = xw.select(0, d);
      f32mm(xc, I, 1, w[d].W, G * H, 1, xwd, G * H, B * T, G * H, I, 0.f,
            w[d].b.defined() ? w[d].b.data_ptr<float>() : nullptr);
    }
  }
  at::Tensor hs = at::empty({nd, B, T + 1, H}, opt);
  at::Tensor cs = c == 1 ? at::empty({nd, B, T + 1, H}, opt) : at::empty({0}, opt);
  at::Tensor gates = at::empty({nd, B, T, G * H}, opt);
  const int64_t Hy = merge == 1 ? 2 * H : H;  // output width
  at::Tensor y = rs ? at::empty({B, T, Hy}, opt) : at::empty({B, Hy}, opt);
  at::Tensor parts;  // sum / ave: the two directions' outputs, merged below
  if (merge >= 2) parts = at::empty({2, y.numel()}, opt);
  RnnDir dr{};
  for (int d = 0; d < nd; ++d) {
    dr.xw[d] = xw.defined() ? xw.data_ptr<float>() + d * B * T * G * H : nullptr;
    dr.W[d] = w[d].W.data_ptr<float>();
    dr.b[d] = w[d].b.defined() ? w[d].b.data_ptr<float>() : nullptr;
    dr.U[d] = w[d].U.data_ptr<float>();
    dr.hs[d] = hs.data_ptr<float>() + d * B * (T + 1) * H;
    dr.cs[d] = c == 1 ? cs.data_ptr<float>() + d * B * (T + 1) * H : nullptr;
    dr.gates[d] = gates.data_ptr<float>() + d * B * T * G * H;
    dr.y[d] = merge >= 2 ? parts.data_ptr<float>() + d * y.numel() : y.data_ptr<float>();
    dr.rev[d] = rev[d];
    dr.yoff[d] = merge == 1 ? d * (int)H : 0;
    dr.yproc[d] = yproc ? 1 : 0;
    dr.rdp[d] = drop.rdp.empty() ? nullptr : drop.rdp[d].data_ptr<float>();
  }
  dr.ldy = (int)Hy;
  dr.dscale = 1.f;
  dr.mask = mk;
  int e = rnn_fwd_dir(c, dr, nd, xc.data_ptr<float>(), (int)I, (int)B, (int)T, (int)H, rs ? 1 : 0, (int)act, (int)ract,
                      cur_stream());
  TORCH_CHECK(e == 0, "rnn_fwd launch failed: ", hipGetErrorString((hipError_t)e));
  if (merge >= 2) {
    e = bidir_merge(parts.data_ptr<float>(), parts.data_ptr<float>() + y.numel(), y.data_ptr<float>(), y.numel(),
                    merge == 3 ? 0.5f : 1.f, cur_stream());
    TORCH_CHECK(e == 0, "bidir_merge launch failed: ", hipGetErrorString((hipError_t)e));
  }
  py::list saved;
  saved.append(hs);
  saved.append(cs);
  saved.append(gates);
  return py::make_tuple(y, saved);
}

// one direction's parameter gradients from its dgates: accumulated into the given fp32 buffers (returns Nones) or
// returned in fresh ones
py::tuple dir_param_grads(int c, const at::Tensor& dg, const at::Tensor& hs, const at::Tensor& gates,
                          const at::Tensor& xc, bool has_b, int rev, const at::Tensor& gW, const at::Tensor& gU,
                          const at::Tensor& gb, int64_t B, int64_t T, int64_t I, int64_t H,
                          const float* dp = nullptr, const float* rdp = nullptr) {
  const int G = gates_of(c);
  const bool dropm = dp || rdp;  // per-gate tiles with the masks on the A rows: every cell and width
  const bool tiles = dropm || c != 0 || (2 * H) % 64 == 0;
  auto param_grad = [&](float* pU, float* pW, float* pb) {
    const int e = dropm ? rnn_param_grad_drop(c, dg.data_ptr<float>(), hs.data_ptr<float>(), gates.data_ptr<float>(),
                                              xc.data_ptr<float>(), dp, rdp, pU, pW, pb, (int)B, (int)T, (int)H, (int)I,
                                              cur_stream(), rev)
                        : rnn_param_grad(c, dg.data_ptr<float>(), hs.data_ptr<float>(), gates.data_ptr<float>(),
                                         xc.data_ptr<float>(), pU, pW, pb, (int)B, (int)T, (int)H, (int)I, cur_stream(),
                                         rev);
    TORCH_CHECK(e == 0, "rnn_param_grad launch failed: ", hipGetErrorString((hipError_t)e));
  };
  if (tiles && gU.defined() && gW.defined() && gb.defined() == has_b) {
    for (const at::Tensor* t : {&gU, &gW})
      TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous(), "rnn_bwd: fp32 contiguous grad buffers");
    TORCH_CHECK(gU.numel() == H * G * H && gW.numel() == I * G * H, "rnn_bwd: grad buffer sizes");
    if (has_b) TORCH_CHECK(gb.scalar_type() == at::kFloat && gb.numel() == G * H, "rnn_bwd: bias grad buffer");
    param_grad(gU.data_ptr<float>(), gW.data_ptr<float>(), has_b ? gb.data_ptr<float>() : nullptr);
    return py::make_tuple(py::none(), py::none(), py::none());
  }
  at::Tensor dW = at::zeros({I, G * H}, xc.options());
  at::Tensor dU = at::zeros({H, G * H}, xc.options());
  at::Tensor db = has_b ? at::zeros({G * H}, xc.options()) : at::Tensor();
  if (tiles) {
    param_grad(dU.data_ptr<float>(), dW.data_ptr<float>(), has_b ? db.data_ptr<float>() : nullptr);
  } else {
    // GRU with 2H not a multiple of 64 (as rnn_bwd_): h_{t-1} is slot t + rev of the saved sequence
    at::Tensor hp = hs.narrow(1, rev, T).contiguous().view({B * T, H});
    at::Tensor rh = gates.view({B * T, G * H}).narrow(1, H, H).mul(hp).contiguous();
    f32mm(xc, 1, I, dg, G * H, 1, dW, G * H, I, G * H, B * T);
    f32mm(hp, 1, H, dg, G * H, 1, dU, G * H, H, 2 * H, B * T);
    at::Tensor dUh = dU.narrow(1, 2 * H, H);
    at::Tensor dgh = dg.narrow(1, 2 * H, H);
    const int e2 = gemm_f32(rh.data_ptr<float>(), 1, H, dgh.data_ptr<float>(), G * H, 1, dUh.data_ptr<float>(), G * H,
                            (int)H, (int)H, (int)(B * T), 1.f, 0.f, nullptr, 0, cur_stream());
    TORCH_CHECK(e2 == 0, "gemm_f32 launch failed");
    if (has_b) {
      const int e3 = colsum_f32(dg.data_ptr<float>(), db.data_ptr<float>(), B * T, (int)(G * H), cur_stream());
      TORCH_CHECK(e3 == 0, "colsum_f32 launch failed");
    }
  }
  return py::make_tuple(dW, dU, db.defined() ? py::cast(db) : py::none());
}

// Returns (dx | None, [(dW, dU, db) per direction]) with None for what went into the given gradient buffers.
py::tuple dir_bwd(int c, const at::Tensor& dy, const at::Tensor& x, const std::vector<DirWeights>& w,
                  const std::vector<int>& rev, bool rs, int merge, bool yproc, const std::vector<at::Tensor>& saved,
                  const std::vector<DirWeights>& gr, bool need_dx, int64_t act, int64_t ract,
                  const c10::optional<at::Tensor>& mask, const DropSet& drop = {}) {
  const int G = gates_of(c);
  const int nd = (int)w.size();
  TORCH_CHECK(x.is_cuda() && x.dim() == 3, "rnn_bwd: x [B,T,I] on GPU");
  const int64_t B = x.size(0), T = x.size(1), I = x.size(2), H = w[0].U.size(0);
  const unsigned char* mk = mask_ptr(mask, x, "rnn_bwd");
  const bool reg = rnn_reg_path(c, (int)H, (int)act, (int)ract);
  TORCH_CHECK(saved.size() == 3, "rnn_bwd: saved = [hs, cs, gates]");
  const at::Tensor& hs = saved[0];
  const at::Tensor& cs = saved[1];
  const at::Tensor& gates = saved[2];
  TORCH_CHECK(hs.numel() == nd * B * (T + 1) * H && gates.numel() == nd * B * T * G * H &&
                  (c != 1 || cs.numel() == hs.numel()), "rnn_bwd: saved tensor sizes");
  const int64_t Hy = merge == 1 ? 2 * H : H;
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kFloat && dy.numel() == (rs ? B * T * Hy : B * Hy),
              "rnn_bwd: dy does not match the output");
  at::DeviceGuard g(x.device());
  at::Tensor dyc = dy.contiguous(), xc = x.contiguous();
  at::Tensor UT;
  if (!reg) {  // the generic kernels read U^T [GH][H]
    UT = at::empty({nd, G * H, H}, x.options());
    for (int d = 0; d < nd; ++d) {
      const int et = transpose_f32(w[d].U.data_ptr<float>(), UT.data_ptr<float>() + d * G * H * H, (int)H, (int)(G * H),
                                   cur_stream());
      TORCH_CHECK(et == 0, "transpose_f32 launch failed");
    }
  }
  at::Tensor dgates = at::empty({nd, B * T, G * H}, x.options());
  RnnDir dr{};
  for (int d = 0; d < nd; ++d) {
    dr.U[d] = w[d].U.data_ptr<float>();
    dr.UT[d] = UT.defined() ? UT.data_ptr<float>() + d * G * H * H : nullptr;
    dr.hs[d] = hs.data_ptr<float>() + d * B * (T + 1) * H;
    dr.cs[d] = c == 1 ? cs.data_ptr<float>() + d * B * (T + 1) * H : nullptr;
    dr.gates[d] = gates.data_ptr<float>() + d * B * T * G * H;
    dr.dgates[d] = dgates.data_ptr<float>() + d * B * T * G * H;
    dr.dy[d] = dyc.data_ptr<float>();
    dr.rev[d] = rev[d];
    dr.yoff[d] = merge == 1 ? d * (int)H : 0;
    dr.yproc[d] = yproc ? 1 : 0;
    dr.rdp[d] = drop.rdp.empty() ? nullptr : drop.rdp[d].data_ptr<float>();
  }
  dr.ldy = (int)Hy;
  dr.dscale = merge == 3 ? 0.5f : 1.f;
  dr.mask = mk;
  const int e = rnn_bwd_dir(c, dr, nd, (int)B, (int)T, (int)H, rs ? 1 : 0, (int)act, (int)ract, cur_stream());
  TORCH_CHECK(e == 0, "rnn_bwd launch failed: ", hipGetErrorString((hipError_t)e));
  py::object dx = py::none();
  if (need_dx) {  // dx[bt][i] = sum_d sum_j dg_d[bt][j] W_d[i][j]: the second direction accumulates
    at::Tensor dxt = at::empty({B * T, I}, x.options());
    if (!drop.dp.empty()) {  // dx[bt] = sum_d sum_g (dg_{d,g}[bt] W_{d,g}^T) * dp_d[g][b]
      at::Tensor tg = at::empty({G, B * T, I}, x.options());
      for (int d = 0; d < nd; ++d) {
        for (int g = 0; g < G; ++g) {
          const int e2 = gemm_f32(dgates.data_ptr<float>() + d * B * T * G * H + g * H, G * H, 1,
                                  w[d].W.data_ptr<float>() + g * H, 1, G * H, tg.data_ptr<float>() + g * B * T * I, I,
                                  (int)(B * T), (int)I, (int)H, 1.f, 0.f, nullptr, 0, cur_stream());
          TORCH_CHECK(e2 == 0, "gemm_f32 launch failed: ", hipGetErrorString((hipError_t)e2));
        }
        const int e3 = rnn_drop_dx(tg.data_ptr<float>(), drop.dp[d].data_ptr<float>(), dxt.data_ptr<float>(), G, (int)B,
                                   (int)T, (int)I, d ? 1 : 0, cur_stream());
        TORCH_CHECK(e3 == 0, "rnn_drop_dx launch failed: ", hipGetErrorString((hipError_t)e3));
      }
    } else {
      for (int d = 0; d < nd; ++d) f32mm(dgates.select(0, d), G * H, 1, w[d].W, 1, G * H, dxt, I, B * T, I, G * H, d ? 1.f : 0.f);
    }
    dx = py::cast(dxt.view({B, T, I}));
  }
  py::list pg;
  for (int d = 0; d < nd; ++d)
    pg.append(dir_param_grads(c, dgates.select(0, d), hs.select(0, d), gates.select(0, d), xc, w[d].b.defined(), rev[d],
                              gr[d].W, gr[d].U, gr[d].b, B, T, I, H,
                              drop.dp.empty() ? nullptr : drop.dp[d].data_ptr<float>(),
                              drop.rdp.empty() ? nullptr : drop.rdp[d].data_ptr<float>()));
  return py::make_tuple(dx, pg);
}

at::Tensor opt_tensor(const py::handle& o) { return o.is_none() ? at::Tensor() : o.cast<at::Tensor>(); }

py::tuple birnn_fwd_(const std::string& cell, const at::Tensor& x, py::list Ws, py::list Us, py::list bs, bool rs,
                     const std::string& merge, int64_t act, int64_t ract, c10::optional<at::Tensor> mask,
                     std::vector<c10::optional<at::Tensor>> dps, std::vector<c10::optional<at::Tensor>> rdps) {
  const int c = cell_id(cell);
  TORCH_CHECK(Ws.size() == 2, "birnn_fwd: [forward, backward] weights");
  std::vector<DirWeights> w = dir_weights(Ws, Us, bs, x.size(2), gates_of(c));
  const DropSet drop = drop_set(dps, rdps, x, gates_of(c), w[0].U.size(0), 2, "birnn_fwd");
  return dir_fwd(c, x, w, {0, 1}, rs, merge_id(merge), false, act, ract, mask, drop);
}

py::tuple birnn_bwd_(const std::string& cell, const at::Tensor& dy, const at::Tensor& x, py::list Ws, py::list Us,
                     py::list bs, bool rs, const std::string& merge, std::vector<at::Tensor> saved, py::list gWs,
                     py::list gUs, py::list gbs, bool need_dx, int64_t act, int64_t ract,
                     c10::optional<at::Tensor> mask, std::vector<c10::optional<at::Tensor>> dps,
                     std::vector<c10::optional<at::Tensor>> rdps) {
  const int c = cell_id(cell);
  TORCH_CHECK(Ws.size() == 2 && gWs.size() == 2 && gUs.size() == 2 && gbs.size() == 2,
              "birnn_bwd: [forward, backward] weights and gradient buffers");
  std::vector<DirWeights> gr(2);
  for (int d = 0; d < 2; ++d) gr[d] = {opt_tensor(gWs[d]), opt_tensor(gUs[d]), opt_tensor(gbs[d])};
  std::vector<DirWeights> w = dir_weights(Ws, Us, bs, x.size(2), gates_of(c));
  const DropSet drop = drop_set(dps, rdps, x, gates_of(c), w[0].U.size(0), 2, "birnn_bwd");
  return dir_bwd(c, dy, x, w, {0, 1}, rs, merge_id(merge), false, saved, gr, need_dx, act, ract, mask, drop);
}

// reverse: the sequence is processed last-to-first (go_backwards).  y_input_order: a returned sequence (and its
// gradient) is in input time order; default is Keras' processing order.  Both default to the forward layer.
// mask: uint8 [B, T] step mask (1 = data); a masked layer runs the directed kernels, forward as one direction.
// dropout_mask / recurrent_dropout_mask: fp32 [G, B, I] / [G, B, H] multipliers (ddl_ops.h); a call with either runs
// the directed kernels too.
py::tuple rnn_fwd_(const std::string& cell, const at::Tensor& x, const at::Tensor& W, const at::Tensor& U,
                   c10::optional<at::Tensor> b, bool rs, int64_t act, int64_t ract, bool reverse, bool y_input_order,
                   c10::optional<at::Tensor> mask, c10::optional<at::Tensor> dmask, c10::optional<at::Tensor> rmask) {
  const int c = cell_id(cell);
  const int G = gates_of(c);
  if (reverse || mask || dmask || rmask) {
    TORCH_CHECK(x.dim() == 3, "rnn_fwd: x [B,T,I] fp32 on GPU");
    py::list Ws, Us, bs;
    Ws.append(W);
    Us.append(U);
    bs.append(b ? py::cast(*b) : py::none());
    std::vector<DirWeights> w = dir_weights(Ws, Us, bs, x.size(2), G);
    const DropSet drop = drop_set({dmask}, {rmask}, x, G, w[0].U.size(0), 1, "rnn_fwd");
    return dir_fwd(c, x, w, {reverse ? 1 : 0}, rs, 0, !y_input_order, act, ract, mask, drop);
  }
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 3, "rnn_fwd: x [B,T,I] fp32 on GPU");
  const int64_t B = x.size(0), T = x.size(1), I = x.size(2), H = U.size(0);
  TORCH_CHECK(W.size(0) == I && W.size(1) == G * H && U.size(1) == G * H, "rnn_fwd: W [I,GH], U [H,GH]");
  TORCH_CHECK(W.scalar_type() == at::kFloat && U.scalar_type() == at::kFloat, "rnn_fwd: fp32 weights");
  at::DeviceGuard g(x.device());
  at::Tensor xc = x.contiguous(), Wc = W.contiguous();
  at::Tensor bc = b ? b->contiguous() : at::Tensor();
  at::Tensor xw;
  const bool reg = rnn_reg_path(c, (int)H, (int)act, (int)ract);
  if (!(reg && rnn_fuses_input((int)H, (int)I))) {  // wide inputs / generic kernels: one projection GEMM first
    xw = at::empty({B * T, G * H}, x.options());
    f32mm(xc, I, 1, Wc, G * H, 1, xw, G * H, B * T, G * H, I, 0.f, bc.defined() ? bc.data_ptr<float>() : nullptr);
  }
  auto opt = x.options();
  at::Tensor hs = at::empty({B, T + 1, H}, opt);
  at::Tensor cs = c == 1 ? at::empty({B, T + 1, H}, opt) : at::empty({0}, opt);
  at::Tensor gates = at::empty({B, T, G * H}, opt);
  at::Tensor y = rs ? at::empty({B, T, H}, opt) : at::empty({B, H}, opt);
  at::Tensor Uc = U.contiguous();
  int e = rnn_fwd(c, xw.defined() ? xw.data_ptr<float>() : nullptr, xc.data_ptr<float>(), Wc.data_ptr<float>(),
                  bc.defined() ? bc.data_ptr<float>() : nullptr, (int)I, Uc.data_ptr<float>(), hs.data_ptr<float>(),
                  c == 1 ? cs.data_ptr<float>() : nullptr, gates.data_ptr<float>(), y.data_ptr<float>(), (int)B,
                  (int)T, (int)H, rs ? 1 : 0, (int)act, (int)ract, cur_stream());
  TORCH_CHECK(e == 0, "rnn_fwd launch failed: ", hipGetErrorString((hipError_t)e));
  py::list saved;
  saved.append(hs);
  saved.append(cs);
  saved.append(gates);
  return py::make_tuple(y, saved);
}

// Returns (dx | None, dW | None, dU | None, db | None).  On the fast path the parameter
// gradients are accumulated into gW / gU / gb (fp32 arena slices) in-kernel and None is
// returned for them; dx is only computed when need_dx.
py::tuple rnn_bwd_(const std::string& cell, const at::Tensor& dy, const at::Tensor& x, const at::Tensor& W,
                   const at::Tensor& U, c10::optional<at::Tensor> b, bool rs, std::vector<at::Tensor> saved,
                   c10::optional<at::Tensor> gW, c10::optional<at::Tensor> gU, c10::optional<at::Tensor> gb,
                   bool need_dx, int64_t act, int64_t ract, bool reverse, bool y_input_order,
                   c10::optional<at::Tensor> mask, c10::optional<at::Tensor> dmask, c10::optional<at::Tensor> rmask) {
  const int c = cell_id(cell);
  const int G = gates_of(c);
  if (reverse || mask || dmask || rmask) {
    TORCH_CHECK(x.dim() == 3, "rnn_bwd: x [B,T,I] fp32 on GPU");
    py::list Ws, Us, bs;
    Ws.append(W);
    Us.append(U);
    bs.append(b ? py::cast(*b) : py::none());
    std::vector<DirWeights> gr(1);
    gr[0] = {gW ? *gW : at::Tensor(), gU ? *gU : at::Tensor(), gb ? *gb : at::Tensor()};
    std::vector<DirWeights> w = dir_weights(Ws, Us, bs, x.size(2), G);
    const DropSet drop = drop_set({dmask}, {rmask}, x, G, w[0].U.size(0), 1, "rnn_bwd");
    py::tuple r = dir_bwd(c, dy, x, w, {reverse ? 1 : 0}, rs, 0, !y_input_order, saved, gr, need_dx, act, ract, mask,
                          drop);
    py::tuple pg = r[1].cast<py::list>()[0].cast<py::tuple>();
    return py::make_tuple(r[0], pg[0], pg[1], pg[2]);
  }
  const bool reg = rnn_reg_path(c, (int)U.size(0), (int)act, (int)ract);
  const int64_t B = x.size(0), T = x.size(1), I = x.size(2), H = U.size(0);
  TORCH_CHECK(saved.size() == 3, "rnn_bwd: saved = [hs, cs, gates]");
  const at::Tensor& hs = saved[0];
  const at::Tensor& cs = saved[1];
  const at::Tensor& gates = saved[2];
  at::DeviceGuard g(x.device());
  at::Tensor dyc = dy.contiguous();
  at::Tensor Uc = U.contiguous();
  at::Tensor UT = Uc;
  if (!reg) {  // the generic kernels read U^T [GH][H]
    UT = at::empty({G * H, H}, U.options());
    const int et = transpose_f32(Uc.data_ptr<float>(), UT.data_ptr<float>(), (int)H, (int)(G * H), cur_stream());
    TORCH_CHECK(et == 0, "transpose_f32 launch failed");
  }
  at::Tensor dgates = at::empty({B, T, G * H}, x.options());
  int e = rnn_bwd(c, dyc.data_ptr<float>(), Uc.data_ptr<float>(), UT.data_ptr<float>(), hs.data_ptr<float>(),
                  c == 1 ? cs.data_ptr<float>() : nullptr, gates.data_ptr<float>(), dgates.data_ptr<float>(), (int)B,
                  (int)T, (int)H, rs ? 1 : 0, (int)act, (int)ract, cur_stream());
  TORCH_CHECK(e == 0, "rnn_bwd launch failed: ", hipGetErrorString((hipError_t)e));
  at::Tensor dg = dgates.view({B * T, G * H});
  at::Tensor xc = x.contiguous();
  py::object dx = py::none();
  at::Tensor Wc = W.contiguous();
  if (need_dx) {  // dx[bt][i] = sum_j dg[bt][j] W[i][j]
    at::Tensor dxt = at::empty({B * T, I}, x.options());
    f32mm(dg, G * H, 1, Wc, 1, G * H, dxt, I, B * T, I, G * H);
    dx = py::cast(dxt.view({B, T, I}));
  }
  const bool fused = (c != 0 || (2 * H) % 64 == 0) && gU && gW && (gb.has_value() == b.has_value());
  if (fused) {
    for (const auto* t : {&*gU, &*gW})
      TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous(), "rnn_bwd: fp32 contiguous grad buffers");
    TORCH_CHECK(gU->numel() == H * G * H && gW->numel() == I * G * H, "rnn_bwd: grad buffer sizes");
    if (gb) TORCH_CHECK(gb->scalar_type() == at::kFloat && gb->numel() == G * H, "rnn_bwd: bias grad buffer");
    e = rnn_param_grad(c, dg.data_ptr<float>(), hs.data_ptr<float>(), gates.data_ptr<float>(), xc.data_ptr<float>(),
                       gU->data_ptr<float>(), gW->data_ptr<float>(), gb ? gb->data_ptr<float>() : nullptr, (int)B,
                       (int)T, (int)H, (int)I, cur_stream());
    TORCH_CHECK(e == 0, "rnn_param_grad launch failed: ", hipGetErrorString((hipError_t)e));
    return py::make_tuple(dx, py::none(), py::none(), py::none());
  }
  // unfused parameter gradients (no arena buffers given, or a GRU whose H does not tile): the
  // same one-launch kernel into fresh zeroed buffers
  at::Tensor dW = at::zeros({I, G * H}, x.options());
  at::Tensor dU = at::zeros({H, G * H}, x.options());
  at::Tensor db = b ? at::zeros({G * H}, x.options()) : at::Tensor();
  if (c != 0 || (2 * H) % 64 == 0) {
    e = rnn_param_grad(c, dg.data_ptr<float>(), hs.data_ptr<float>(), gates.data_ptr<float>(), xc.data_ptr<float>(),
                       dU.data_ptr<float>(), dW.data_ptr<float>(), b ? db.data_ptr<float>() : nullptr, (int)B, (int)T,
                       (int)H, (int)I, cur_stream());
    TORCH_CHECK(e == 0, "rnn_param_grad launch failed: ", hipGetErrorString((hipError_t)e));
  } else {
    // GRU with 2H not a multiple of 64: dU = [h_{t-1}]^T dg for z,r and [r*h_{t-1}]^T dg for h
    at::Tensor hp = hs.narrow(1, 0, T).contiguous().view({B * T, H});
    at::Tensor rh = gates.view({B * T, G * H}).narrow(1, H, H).mul(hp).contiguous();
    f32mm(xc, 1, I, dg, G * H, 1, dW, G * H, I, G * H, B * T);
    f32mm(hp, 1, H, dg, G * H, 1, dU, G * H, H, 2 * H, B * T);
    at::Tensor dUh = dU.narrow(1, 2 * H, H);
    at::Tensor dgh = dg.narrow(1, 2 * H, H);
    const int e2 = gemm_f32(rh.data_ptr<float>(), 1, H, dgh.data_ptr<float>(), G * H, 1, dUh.data_ptr<float>(), G * H,
                            (int)H, (int)H, (int)(B * T), 1.f, 0.f, nullptr, 0, cur_stream());
    TORCH_CHECK(e2 == 0, "gemm_f32 launch failed");
    if (b) {
      const int e3 = colsum_f32(dg.data_ptr<float>(), db.data_ptr<float>(), B * T, (int)(G * H), cur_stream());
      TORCH_CHECK(e3 == 0, "colsum_f32 launch failed");
    }
  }
  return py::make_tuple(dx, dW, dU, db.defined() ? py::cast(db) : py::none());
}

// Replica-batched training step of R co-located RNN(H) -> Dense(K) / MSE replicas (kernels/rnn.hip,
// rnn_replica_step): every list holds one entry per replica; None entries of the optional lists are
// absent biases / optimizer states.  All tensors fp32, contiguous, on one device.
float* fptr(const py::handle& o, const char* what, int64_t numel = -1) {
  if (o.is_none()) return nullptr;
  at::Tensor t = o.cast<at::Tensor>();
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous(), "rnn_replica_step: ", what,
              " must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(numel < 0 || t.numel() >= numel, "rnn_replica_step: ", what, " too small");
  return t.data_ptr<float>();
}

void rnn_replica_step_(const std::string& cell, py::list xs, py::list ys, py::list Ws, py::list Us, py::list bs,
                       py::list Wds, py::list bds, py::list gWs, py::list gUs, py::list gbs, py::list gWds,
                       py::list gbds, py::list hists, at::Tensor ctr, std::vector<int64_t> nbs,
                       std::vector<int64_t> steps, at::Tensor live, int64_t B, at::Tensor hs,
                       at::Tensor cs, at::Tensor gates, at::Tensor hlast, at::Tensor dh, at::Tensor dgates,
                       py::list ws, py::list gs, py::list s1s, py::list s2s, py::list ts, int64_t opt, double lr,
                       double p1, double p2, double eps, double wd, int64_t amode) {
  const int c = cell_id(cell);
  TORCH_CHECK(c == 0 || c == 1, "rnn_replica_step: GRU or LSTM");
  const int G = gates_of(c);
  const int R = (int)xs.size();
  TORCH_CHECK(R >= 1 && R <= kMaxRnnRep, "rnn_replica_step: 1..", kMaxRnnRep, " replicas");
  for (py::list* l : {&ys, &Ws, &Us, &bs, &Wds, &bds, &gWs, &gUs, &gbs, &gWds, &gbds, &hists, &ws, &gs, &s1s, &s2s, &ts})
    TORCH_CHECK((int)l->size() == R, "rnn_replica_step: one entry per replica in every list");
  at::Tensor x0 = xs[0].cast<at::Tensor>(), U0 = Us[0].cast<at::Tensor>(), Wd0 = Wds[0].cast<at::Tensor>();
  TORCH_CHECK(x0.dim() == 3, "rnn_replica_step: x shards [rows, T, I]");
  const int64_t T = x0.size(1), I = x0.size(2), H = U0.size(0), K = Wd0.size(0);
  TORCH_CHECK(U0.size(1) == G * H && Wd0.size(1) == H, "rnn_replica_step: U [H, GH], Dense kernel [K, H]");
  TORCH_CHECK(rnn_replica_ok(c, (int)H, (int)I, (int)K, (int)B), "rnn_replica_step: unsupported H / I / K / B");
  TORCH_CHECK(ctr.is_cuda() && ctr.scalar_type() == at::kInt && ctr.numel() >= 1, "rnn_replica_step: int32 ctr");
  TORCH_CHECK(live.is_cuda() && live.scalar_type() == at::kInt && live.numel() >= R && live.device() == ctr.device(),
              "rnn_replica_step: int32 live flags [R] on the counter's device");
  TORCH_CHECK((int)nbs.size() == R && (int)steps.size() == R, "rnn_replica_step: batches and steps per replica");
  const int64_t RB = R * B;
  const int64_t n = ws[0].cast<at::Tensor>().numel();
  RnnRep rp{};
  OptRep op{};
  for (int r = 0; r < R; ++r) {
    const int64_t nb = nbs[r];
    TORCH_CHECK(nb >= 1 && steps[r] >= 0 && steps[r] < (1LL << 31), "rnn_replica_step: batches >= 1, steps >= 0");
    rp.nbr[r] = (int)nb;
    rp.steps[r] = (int)steps[r];
    rp.x[r] = fptr(xs[r], "x shard", nb * B * T * I);
    rp.y[r] = fptr(ys[r], "y shard", nb * B * K);
    rp.W[r] = fptr(Ws[r], "W", I * G * H);
    rp.U[r] = fptr(Us[r], "U", H * G * H);
    rp.b[r] = fptr(bs[r], "b", G * H);
    rp.Wd[r] = fptr(Wds[r], "Dense kernel", K * H);
    rp.bd[r] = fptr(bds[r], "Dense bias", K);
    rp.gW[r] = fptr(gWs[r], "gW", I * G * H);
    rp.gU[r] = fptr(gUs[r], "gU", H * G * H);
    rp.gb[r] = fptr(gbs[r], "gb", G * H);
    rp.gWd[r] = fptr(gWds[r], "gWd", K * H);
    rp.gbd[r] = fptr(gbds[r], "gbd", K);
    TORCH_CHECK(!bs[r].is_none() && !gbs[r].is_none(), "rnn_replica_step: recurrent bias required");
    TORCH_CHECK(bds[r].is_none() == gbds[r].is_none(), "rnn_replica_step: Dense bias and its gradient together");
    rp.hist[r] = fptr(hists[r], "history", steps[r]);  // one slot per step the replica takes
    TORCH_CHECK(rp.hist[r], "rnn_replica_step: history required");
    op.w[r] = fptr(ws[r], "weights", n);
    op.g[r] = fptr(gs[r], "grads", n);
    op.s1[r] = fptr(s1s[r], "optimizer state", n);
    op.s2[r] = fptr(s2s[r], "optimizer state 2", n);
    op.t[r] = fptr(ts[r], "step counter", 1);
    TORCH_CHECK(ws[r].cast<at::Tensor>().numel() == n, "rnn_replica_step: equal arena sizes");
    if (opt == 2) TORCH_CHECK(op.s1[r] && op.s2[r] && op.t[r], "rnn_replica_step: Adam needs m, v and t");
    if (opt == 1) TORCH_CHECK(op.s1[r], "rnn_replica_step: Adagrad needs its accumulator");
  }
  rp.ctr = ctr.data_ptr<int>();
  rp.live = live.data_ptr<int>();
  rp.B = (int)B;
  rp.K = (int)K;
  float* hsp = fptr(py::cast(hs), "hs", RB * (T + 1) * H);
  float* csp = c == 1 ? fptr(py::cast(cs), "cs", RB * (T + 1) * H) : nullptr;
  float* gp = fptr(py::cast(gates), "gates", RB * T * G * H);
  float* hl = fptr(py::cast(hlast), "h_last", RB * H);
  float* dhp = fptr(py::cast(dh), "dh", RB * H);
  float* dgp = fptr(py::cast(dgates), "dgates", RB * T * G * H);
  at::DeviceGuard g(x0.device());
  const int e = rnn_replica_step(c, rp, R, (int)T, (int)H, (int)I, hsp, csp, gp, hl, dhp, dgp, op, n, (int)opt,
                                 (float)lr, (float)p1, (float)p2, (float)eps, (float)wd, (int)amode, cur_stream());
  TORCH_CHECK(e == 0, "rnn_replica_step launch failed: ", hipGetErrorString((hipError_t)e));
}

// Step masks (kernels/rnn.hip): returns (y, mask); y is x itself unless apply (mask_value != 0 zeroes masked steps)
py::tuple mask_from_features_(const at::Tensor& x, double mask_value, bool apply) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 3 && x.is_contiguous(),
              "mask_from_features: x [B,T,F] contiguous fp32 on GPU");
  at::DeviceGuard g(x.device());
  at::Tensor mask = at::empty({x.size(0), x.size(1)}, x.options().dtype(at::kByte));
  at::Tensor y = apply ? at::empty_like(x) : x;
  const int e = mask_from_features(x.data_ptr<float>(), apply ? y.data_ptr<float>() : nullptr,
                                   mask.data_ptr<unsigned char>(), x.size(0) * x.size(1), (int)x.size(2),
                                   (float)mask_value, cur_stream());
  TORCH_CHECK(e == 0, "mask_from_features launch failed: ", hipGetErrorString((hipError_t)e));
  return py::make_tuple(y, mask);
}

at::Tensor mask_apply_(const at::Tensor& x, const at::Tensor& mask) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 3 && x.is_contiguous(),
              "mask_apply: x [B,T,F] contiguous fp32 on GPU");
  mask_ptr(mask, x, "mask_apply");
  at::DeviceGuard g(x.device());
  at::Tensor out = at::empty_like(x);
  const int e = mask_apply(x.data_ptr<float>(), mask.data_ptr<unsigned char>(), out.data_ptr<float>(),
                           x.size(0) * x.size(1), (int)x.size(2), cur_stream());
  TORCH_CHECK(e == 0, "mask_apply launch failed: ", hipGetErrorString((hipError_t)e));
  return out;
}

at::Tensor mask_from_ids_(const at::Tensor& ids) {
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == at::kLong && ids.dim() == 2 && ids.is_contiguous(),
              "mask_from_ids: ids [B,T] contiguous int64 on GPU");
  at::DeviceGuard g(ids.device());
  at::Tensor mask = at::empty(ids.sizes(), ids.options().dtype(at::kByte));
  const int e = mask_from_ids(ids.data_ptr<int64_t>(), mask.data_ptr<unsigned char>(), ids.numel(), cur_stream());
  TORCH_CHECK(e == 0, "mask_from_ids launch failed: ", hipGetErrorString((hipError_t)e));
  return mask;
}

}  // namespace

void register_rnn(py::module& m) {
  const std::vector<c10::optional<at::Tensor>> kNoDrop{c10::nullopt, c10::nullopt};  // [forward, backward]: none
  m.def("rnn_fwd", &rnn_fwd_, "persistent GRU/LSTM/SimpleRNN forward (fp32)", py::arg("cell"), py::arg("x"),
        py::arg("W"), py::arg("U"), py::arg("b"), py::arg("rs"), py::arg("act") = (int64_t)ACT_C_TANH,
        py::arg("ract") = (int64_t)ACT_C_HARD_SIGMOID, py::arg("reverse") = false, py::arg("y_input_order") = false,
        py::arg("mask") = py::none(), py::arg("dropout_mask") = py::none(),
        py::arg("recurrent_dropout_mask") = py::none());
  m.def("rnn_bwd", &rnn_bwd_, "persistent GRU/LSTM backward (fp32)", py::arg("cell"), py::arg("dy"), py::arg("x"),
        py::arg("W"), py::arg("U"), py::arg("b"), py::arg("rs"), py::arg("saved"), py::arg("gW") = py::none(),
        py::arg("gU") = py::none(), py::arg("gb") = py::none(), py::arg("need_dx") = true,
        py::arg("act") = (int64_t)ACT_C_TANH, py::arg("ract") = (int64_t)ACT_C_HARD_SIGMOID,
        py::arg("reverse") = false, py::arg("y_input_order") = false, py::arg("mask") = py::none(),
        py::arg("dropout_mask") = py::none(), py::arg("recurrent_dropout_mask") = py::none());
  m.def("birnn_fwd", &birnn_fwd_, "Bidirectional GRU/LSTM/SimpleRNN forward: both directions in one recurrence launch",
        py::arg("cell"), py::arg("x"), py::arg("Ws"), py::arg("Us"), py::arg("bs"), py::arg("rs"),
        py::arg("merge") = "concat", py::arg("act") = (int64_t)ACT_C_TANH,
        py::arg("ract") = (int64_t)ACT_C_HARD_SIGMOID, py::arg("mask") = py::none(),
        py::arg("dropout_masks") = kNoDrop, py::arg("recurrent_dropout_masks") = kNoDrop);
  m.def("birnn_bwd", &birnn_bwd_, "Bidirectional backward: one recurrence launch, parameter gradients per direction",
        py::arg("cell"), py::arg("dy"), py::arg("x"), py::arg("Ws"), py::arg("Us"), py::arg("bs"), py::arg("rs"),
        py::arg("merge"), py::arg("saved"), py::arg("gWs"), py::arg("gUs"), py::arg("gbs"), py::arg("need_dx") = true,
        py::arg("act") = (int64_t)ACT_C_TANH, py::arg("ract") = (int64_t)ACT_C_HARD_SIGMOID,
        py::arg("mask") = py::none(), py::arg("dropout_masks") = kNoDrop,
        py::arg("recurrent_dropout_masks") = kNoDrop);
  m.def("mask_from_features", &mask_from_features_, "step mask any_f(x != mask_value) of x [B,T,F]; y = x * mask",
        py::arg("x"), py::arg("mask_value"), py::arg("apply"));
  m.def("mask_apply", &mask_apply_, "out = in * mask[..., None] (the Masking gradient)", py::arg("x"), py::arg("mask"));
  m.def("mask_from_ids", &mask_from_ids_, "step mask ids != 0 of int64 token ids [B,T]", py::arg("ids"));
  m.def("rnn_replica_step", &rnn_replica_step_, "one training step of R co-located RNN -> Dense / MSE replicas");
  m.def("rnn_replica_ok", [](const std::string& cell, int64_t H, int64_t I, int64_t K, int64_t B) {
    return rnn_replica_ok(cell_id(cell), (int)H, (int)I, (int)K, (int)B);
  });
}
