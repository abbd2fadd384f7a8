// Python bindings for the gfx950 HIP op library.
#include <torch/extension.h>

#include <vector>

std::vector<at::Tensor> layernorm_fwd(at::Tensor x, at::Tensor w,
                                      at::Tensor b, double eps);
std::vector<at::Tensor> layernorm_bwd(at::Tensor dy, at::Tensor x,
                                      at::Tensor w, at::Tensor mean,
                                      at::Tensor rstd);
at::Tensor geglu_fwd(at::Tensor x);
at::Tensor geglu_bwd(at::Tensor dy, at::Tensor x);
std::vector<at::Tensor> geglu_bwd_colsum(at::Tensor dy, at::Tensor x);
long geglu_bwd_colsum_max_h();
at::Tensor dist_buckets(at::Tensor coords, at::Tensor boundaries);
at::Tensor pcgemm(at::Tensor A, at::Tensor B, long Bb, long M, long N,
                  long K, long D,
                  long a_bs, long a_ms, long a_ks,
                  long b_bs, long b_ns, long b_ks, double alpha,
                  long variant);
at::Tensor gatemul_fwd(at::Tensor x, at::Tensor g, long xs, long gs,
                       c10::optional<at::Tensor> rowmask);
std::vector<at::Tensor> gatemul_bwd(at::Tensor dy, at::Tensor x, at::Tensor g,
                                    long xs, long gs,
                                    c10::optional<at::Tensor> rowmask,
                                    c10::optional<at::Tensor> dx_out,
                                    c10::optional<at::Tensor> dg_out,
                                    long dxs, long dgs);
at::Tensor linear_fwd(at::Tensor x, at::Tensor W,
                      c10::optional<at::Tensor> bias,
                      c10::optional<at::Tensor> resid, long stage);
std::vector<at::Tensor> ff1_geglu_fwd(at::Tensor x, at::Tensor W,
                                      c10::optional<at::Tensor> bias,
                                      long stage, bool want_inter);
at::Tensor wgrad(at::Tensor dY, at::Tensor X);
at::Tensor wgrad_v1(at::Tensor dY, at::Tensor X);
std::vector<at::Tensor> wgrad_colsum(at::Tensor dY, at::Tensor X);
std::vector<at::Tensor> ipa_core_fwd(
    at::Tensor q_s, at::Tensor k_s, at::Tensor v_s, at::Tensor q_pg,
    at::Tensor k_pg, at::Tensor v_pg, at::Tensor bias, at::Tensor pair,
    at::Tensor rot, at::Tensor trans, at::Tensor point_w, double scale_s,
    double scale_b, double scale_p, double eps,
    c10::optional<at::Tensor> mask, bool save_stats);
std::vector<at::Tensor> ipa_core_bwd(
    at::Tensor dout, at::Tensor attn, at::Tensor gpts, at::Tensor q_s,
    at::Tensor k_s, at::Tensor v_s, at::Tensor q_pg, at::Tensor k_pg,
    at::Tensor v_pg, at::Tensor bias, at::Tensor pair, at::Tensor rot,
    at::Tensor trans, at::Tensor point_w, double scale_s, double scale_b,
    double scale_p, double eps, c10::optional<at::Tensor> mask,
    bool need_dpair, bool need_drot);
long ipa_core_max_n(long heads, long pair_dim);
std::vector<at::Tensor> se3_core_fwd(
    at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor x,
    at::Tensor edges, at::Tensor w_e, at::Tensor b_e, double scale,
    double eps, c10::optional<at::Tensor> mask, bool save_attn);
std::vector<at::Tensor> se3_core_bwd(
    at::Tensor dout, at::Tensor ddxh, at::Tensor attn, at::Tensor q,
    at::Tensor k, at::Tensor v, at::Tensor x, at::Tensor edges,
    at::Tensor w_e, at::Tensor b_e, double scale, double eps,
    c10::optional<at::Tensor> mask, bool need_dedges);
long se3_core_max_n(long heads, long dim_head, long edge_dim);
std::vector<at::Tensor> egnn_core_fwd(
    at::Tensor P, at::Tensor Q, at::Tensor x, at::Tensor edges,
    at::Tensor W_e, at::Tensor w_d, at::Tensor W2, at::Tensor b2,
    at::Tensor Wc1, at::Tensor bc1, at::Tensor Wc2, at::Tensor bc2,
    double eps, c10::optional<at::Tensor> mask);
std::vector<at::Tensor> egnn_core_bwd(
    at::Tensor dm, at::Tensor ddx, at::Tensor P, at::Tensor Q, at::Tensor x,
    at::Tensor edges, at::Tensor W_e, at::Tensor w_d, at::Tensor W2,
    at::Tensor b2, at::Tensor Wc1, at::Tensor bc1, at::Tensor Wc2,
    at::Tensor bc2, double eps, c10::optional<at::Tensor> mask);
long egnn_core_max_edge_dim();
at::Tensor pairrep_fwd(at::Tensor left, at::Tensor right, at::Tensor emb,
                       at::Tensor rel);
bool pairrep_bwd_covers(at::Tensor dy, long emb_rows);
std::vector<at::Tensor> pairrep_bwd(at::Tensor dy, at::Tensor rel,
                                    long emb_rows);
at::Tensor colsum_fold(at::Tensor part,
                       c10::optional<at::Tensor> accumulate_into, bool v1);
std::vector<at::Tensor> attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 c10::optional<at::Tensor> bias,
                                 c10::optional<at::Tensor> mask,
                                 long bias_repeat, double scale,
                                 long q_repeat, double dropout_p,
                                 c10::optional<at::Tensor> rng_state);
at::Tensor attn_dropout_mask(at::Tensor rng_state, long B, long H, long Lq,
                             long Lk, double dropout_p);
std::vector<at::Tensor> attn_bwd(at::Tensor dout, at::Tensor q, at::Tensor k,
                                 at::Tensor v, at::Tensor out, at::Tensor lse,
                                 c10::optional<at::Tensor> bias,
                                 c10::optional<at::Tensor> mask,
                                 long bias_repeat, double scale,
                                 bool need_dbias, long q_repeat,
                                 c10::optional<at::Tensor> dq_out,
                                 c10::optional<at::Tensor> dk_out,
                                 c10::optional<at::Tensor> dv_out,
                                 double dropout_p,
                                 c10::optional<at::Tensor> rng_state,
                                 c10::optional<int64_t> ds_scratch_bytes,
                                 c10::optional<at::Tensor> delta,
                                 c10::optional<int64_t> dq_entries_per_block);
std::vector<at::Tensor> attn_gate_bwd(at::Tensor dy, at::Tensor out,
                                      at::Tensor g, at::Tensor dg_out,
                                      bool want_colsum);
std::vector<at::Tensor> tplattn_fwd(at::Tensor q, at::Tensor kv, long heads,
                                    c10::optional<at::Tensor> key_mask,
                                    c10::optional<at::Tensor> query_mask);
std::vector<at::Tensor> tplattn_bwd(at::Tensor dout, at::Tensor q,
                                    at::Tensor kv, at::Tensor out,
                                    at::Tensor lse, long heads,
                                    c10::optional<at::Tensor> key_mask,
                                    c10::optional<at::Tensor> query_mask);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("layernorm_fwd", &layernorm_fwd, "fused LayerNorm forward (gfx950)");
  m.def("layernorm_bwd", &layernorm_bwd, "fused LayerNorm backward (gfx950)");
  m.def("geglu_fwd", &geglu_fwd, "fused GEGLU forward (gfx950)");
  m.def("geglu_bwd", &geglu_bwd, "fused GEGLU backward (gfx950)");
  m.def("geglu_bwd_colsum", &geglu_bwd_colsum,
        "fused GEGLU backward -> [dx, fp32 column sum of the rounded dx] "
        "(gfx950, bf16)", py::arg("dy"), py::arg("x"));
  m.def("geglu_bwd_colsum_max_h", &geglu_bwd_colsum_max_h,
        "largest half width geglu_bwd_colsum covers");
  m.def("dist_buckets", &dist_buckets, "fused cdist+bucketize (gfx950)");
  m.def("pcgemm", &pcgemm,
        "per-channel batched GEMM, stride-parameterized (gfx950 MFMA); "
        "variant 1 = scatter staging, 2 = wide stores, 3 = full lines, "
        "0 = default",
        py::arg("A"), py::arg("B"), py::arg("Bb"), py::arg("M"), py::arg("N"),
        py::arg("K"), py::arg("D"), py::arg("a_bs"), py::arg("a_ms"),
        py::arg("a_ks"), py::arg("b_bs"), py::arg("b_ns"), py::arg("b_ks"),
        py::arg("alpha"), py::arg("variant") = 0);
  m.def("gatemul_fwd", &gatemul_fwd, "fused x*sigmoid(g) forward (gfx950)",
        py::arg("x"), py::arg("g"), py::arg("xs"), py::arg("gs"),
        py::arg("rowmask") = c10::nullopt);
  m.def("gatemul_bwd", &gatemul_bwd, "fused x*sigmoid(g) backward (gfx950)",
        py::arg("dy"), py::arg("x"), py::arg("g"), py::arg("xs"),
        py::arg("gs"), py::arg("rowmask") = c10::nullopt,
        py::arg("dx_out") = c10::nullopt, py::arg("dg_out") = c10::nullopt,
        py::arg("dxs") = 0, py::arg("dgs") = 0);
  m.def("linear_fwd", &linear_fwd,
        "tall-M small-K linear GEMM, bias/residual epilogue (gfx950 MFMA)",
        py::arg("x"), py::arg("W"), py::arg("bias") = c10::nullopt,
        py::arg("resid") = c10::nullopt, py::arg("stage") = -1);
  m.def("ff1_geglu_fwd", &ff1_geglu_fwd,
        "linear GEMM with fused GEGLU epilogue (gfx950 MFMA)",
        py::arg("x"), py::arg("W"), py::arg("bias") = c10::nullopt,
        py::arg("stage") = -1, py::arg("want_inter") = true);
  m.def("pairrep_fwd", &pairrep_fwd,
        "fused pair-rep build: outer sum + rel-pos embedding gather "
        "(gfx950, K13)", py::arg("left"), py::arg("right"), py::arg("emb"),
        py::arg("rel"));
  m.def("pairrep_bwd", &pairrep_bwd,
        "pair-rep backward from one read of dy -> [dleft, dright, demb], "
        "fp32 sums rounded once; no atomics (gfx950, K13)",
        py::arg("dy"), py::arg("rel"), py::arg("emb_rows"));
  m.def("pairrep_bwd_covers", &pairrep_bwd_covers,
        "whether pairrep_bwd covers dy's shape, dtype and layout on the "
        "current device",
        py::arg("dy"), py::arg("emb_rows"));
  m.def("colsum_fold", &colsum_fold,
        "fixed-order fold of (nb, C) fp32 partial rows -> (C,), or added "
        "into accumulate_into in place; v1 keeps the scalar body",
        py::arg("part"), py::arg("accumulate_into") = c10::nullopt,
        py::arg("v1") = false);
  m.def("ipa_core_fwd", &ipa_core_fwd,
        "fused fp32 IPA attention core forward -> [out, attn, gpts]; attn "
        "and gpts are saved for the backward only with save_stats "
        "(gfx950, K7)",
        py::arg("q_s"), py::arg("k_s"), py::arg("v_s"), py::arg("q_pg"),
        py::arg("k_pg"), py::arg("v_pg"), py::arg("bias"), py::arg("pair"),
        py::arg("rot"), py::arg("trans"), py::arg("point_w"),
        py::arg("scale_s"), py::arg("scale_b"), py::arg("scale_p"),
        py::arg("eps"), py::arg("mask") = c10::nullopt,
        py::arg("save_stats") = false);
  m.def("ipa_core_bwd", &ipa_core_bwd,
        "fused fp32 IPA attention core backward: gradients of the eleven "
        "core inputs, row-side + column-side kernels, no atomics "
        "(gfx950, K7)",
        py::arg("dout"), py::arg("attn"), py::arg("gpts"), py::arg("q_s"),
        py::arg("k_s"), py::arg("v_s"), py::arg("q_pg"), py::arg("k_pg"),
        py::arg("v_pg"), py::arg("bias"), py::arg("pair"), py::arg("rot"),
        py::arg("trans"), py::arg("point_w"), py::arg("scale_s"),
        py::arg("scale_b"), py::arg("scale_p"), py::arg("eps"),
        py::arg("mask") = c10::nullopt, py::arg("need_dpair") = true,
        py::arg("need_drot") = true);
  m.def("ipa_core_max_n", &ipa_core_max_n,
        "largest sequence length whose IPA core forward and backward fit "
        "the device's LDS per block",
        py::arg("heads"), py::arg("pair_dim") = 512);
  m.def("se3_core_fwd", &se3_core_fwd,
        "fused fp32 SE(3) refiner attention core forward -> [out, dxh, "
        "attn]; attn is saved for the backward only with save_attn "
        "(gfx950, K15)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("x"),
        py::arg("edges"), py::arg("w_e"), py::arg("b_e"), py::arg("scale"),
        py::arg("eps"), py::arg("mask") = c10::nullopt,
        py::arg("save_attn") = false);
  m.def("se3_core_bwd", &se3_core_bwd,
        "fused fp32 SE(3) refiner attention core backward: gradients of "
        "the seven core inputs, row-side + column-side kernels, no atomics "
        "(gfx950, K15)",
        py::arg("dout"), py::arg("ddxh"), py::arg("attn"), py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("x"), py::arg("edges"),
        py::arg("w_e"), py::arg("b_e"), py::arg("scale"), py::arg("eps"),
        py::arg("mask") = c10::nullopt, py::arg("need_dedges") = true);
  m.def("se3_core_max_n", &se3_core_max_n,
        "largest sequence length whose SE(3) core forward and backward "
        "fit the device's LDS per block",
        py::arg("heads"), py::arg("dim_head"), py::arg("edge_dim"));
  m.def("egnn_core_fwd", &egnn_core_fwd,
        "fused fp32 EGNN edge-message core forward -> [m_i, dx]; writes "
        "nothing of pair size (gfx950 f32 MFMA, K16)",
        py::arg("P"), py::arg("Q"), py::arg("x"), py::arg("edges"),
        py::arg("W_e"), py::arg("w_d"), py::arg("W2"), py::arg("b2"),
        py::arg("Wc1"), py::arg("bc1"), py::arg("Wc2"), py::arg("bc2"),
        py::arg("eps"), py::arg("mask") = c10::nullopt);
  m.def("egnn_core_bwd", &egnn_core_bwd,
        "fused fp32 EGNN edge-message core backward, recomputing the "
        "forward -> [dP, dQ, dx, dz1, dw_d, dW2, db2, dWc1, dbc1, dWc2, "
        "dbc2]; no atomics (gfx950 f32 MFMA, K16)",
        py::arg("dm"), py::arg("ddx"), py::arg("P"), py::arg("Q"),
        py::arg("x"), py::arg("edges"), py::arg("W_e"), py::arg("w_d"),
        py::arg("W2"), py::arg("b2"), py::arg("Wc1"), py::arg("bc1"),
        py::arg("Wc2"), py::arg("bc2"), py::arg("eps"),
        py::arg("mask") = c10::nullopt);
  m.def("egnn_core_max_edge_dim", &egnn_core_max_edge_dim,
        "largest edge dim whose EGNN core forward and backward fit the "
        "device's LDS per block");
  m.def("wgrad", &wgrad,
        "split-K weight-gradient GEMM dY^T @ X (gfx950 MFMA, fp32 out): "
        "the streaming kernel with a fixed-order fold, or the r02 kernel "
        "under AF2AMD_WGRAD_V1=1",
        py::arg("dY"), py::arg("X"));
  m.def("wgrad_v1", &wgrad_v1,
        "the r02 split-K weight-gradient kernel (fp32 atomic drain)",
        py::arg("dY"), py::arg("X"));
  m.def("wgrad_colsum", &wgrad_colsum,
        "streaming split-K weight gradient -> [dW (M, N), sum_k dY[k, :] "
        "(M,)] fp32 from one pass over dY and X",
        py::arg("dY"), py::arg("X"));
  m.def("attn_fwd", &attn_fwd, "fused flash attention forward (gfx950)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("bias"),
        py::arg("mask"), py::arg("bias_repeat"), py::arg("scale"),
        py::arg("q_repeat") = 1, py::arg("dropout_p") = 0.0,
        py::arg("rng_state") = c10::nullopt);
  m.def("attn_dropout_mask", &attn_dropout_mask,
        "keep mask (B, H, Lq, Lk) uint8 of the fused attention dropout",
        py::arg("rng_state"), py::arg("B"), py::arg("H"), py::arg("Lq"),
        py::arg("Lk"), py::arg("dropout_p"));
  m.def("attn_bwd", &attn_bwd, "fused flash attention backward (gfx950)",
        py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("out"), py::arg("lse"), py::arg("bias"), py::arg("mask"),
        py::arg("bias_repeat"), py::arg("scale"), py::arg("need_dbias"),
        py::arg("q_repeat") = 1,
        py::arg("dq_out") = c10::nullopt, py::arg("dk_out") = c10::nullopt,
        py::arg("dv_out") = c10::nullopt, py::arg("dropout_p") = 0.0,
        py::arg("rng_state") = c10::nullopt,
        // byte cap of the stored-dS scratch; None = AF2AMD_DS_SCRATCH_BYTES
        // (default 2 GiB), 0 = the float-atomic dBias path
        py::arg("ds_scratch_bytes") = c10::nullopt,
        // rowsum(dO * O) as fp32 (B, h, Lq) when the caller already has it
        // (attn_gate_bwd): no attn_delta_kernel is launched
        py::arg("delta") = c10::nullopt,
        // for tests: batch entries per block of the fused dQ + dBias
        // kernel (Lk <= 384); None = automatic (fused up to Lk = 256),
        // 0 = the two kernels (dQ, then the sum)
        py::arg("dq_entries_per_block") = c10::nullopt);
  m.def("attn_gate_bwd", &attn_gate_bwd,
        "gate backward of gated attention in one pass -> [dO, delta"
        "[, colsum]]; dg goes into dg_out, a slice of the packed gradient "
        "(gfx950)",
        py::arg("dy"), py::arg("out"), py::arg("g"), py::arg("dg_out"),
        py::arg("want_colsum") = false);
  m.def("tplattn_fwd", &tplattn_fwd,
        "template pointwise attention forward, one query and T keys per "
        "pair position, operands in their projection layouts -> [out, lse] "
        "(gfx950, bf16 / fp32, K5)",
        py::arg("q"), py::arg("kv"), py::arg("heads"),
        py::arg("key_mask") = c10::nullopt,
        py::arg("query_mask") = c10::nullopt);
  m.def("tplattn_bwd", &tplattn_bwd,
        "template pointwise attention backward -> [dq, dkv]; dkv is one "
        "tensor in kv's layout, no atomics (gfx950, bf16 / fp32, K5)",
        py::arg("dout"), py::arg("q"), py::arg("kv"), py::arg("out"),
        py::arg("lse"), py::arg("heads"),
        py::arg("key_mask") = c10::nullopt,
        py::arg("query_mask") = c10::nullopt);
}
