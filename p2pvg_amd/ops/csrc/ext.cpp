// Python bindings for the p2pvg_amd gfx950 kernel library.
#include <torch/extension.h>

#include <vector>

std::vector<torch::Tensor> lstm_cell_fwd(torch::Tensor x, torch::Tensor h,
                                         torch::Tensor c, torch::Tensor w_ih,
                                         torch::Tensor w_hh, torch::Tensor b_ih,
                                         torch::Tensor b_hh);
std::vector<torch::Tensor> lstm_cell_bwd_pointwise(
    torch::Tensor dh, c10::optional<torch::Tensor> dc_in, torch::Tensor gates,
    torch::Tensor c_prev, torch::Tensor c_new);
void multi_tensor_adam(std::vector<torch::Tensor> params,
                       std::vector<torch::Tensor> grads,
                       std::vector<torch::Tensor> exp_avgs,
                       std::vector<torch::Tensor> exp_avg_sqs, double lr,
                       double beta1, double beta2, double eps,
                       double weight_decay, torch::Tensor step);
torch::Tensor gaussian_kl_fwd(torch::Tensor mu1, torch::Tensor lv1,
                              torch::Tensor mu2, torch::Tensor lv2,
                              double denom);
std::vector<torch::Tensor> gaussian_kl_bwd(torch::Tensor mu1, torch::Tensor lv1,
                                           torch::Tensor mu2, torch::Tensor lv2,
                                           torch::Tensor dout, double denom);

torch::Tensor affine4_fwd(torch::Tensor h, torch::Tensor g, torch::Tensor s1,
                          torch::Tensor s2, torch::Tensor W,
                          c10::optional<torch::Tensor> b);
std::vector<torch::Tensor> affine4_bwd(
    torch::Tensor gout, torch::Tensor h, torch::Tensor g, torch::Tensor s1,
    torch::Tensor s2, torch::Tensor W, c10::optional<torch::Tensor> dW_acc,
    c10::optional<torch::Tensor> db_acc, bool need_dh, bool need_dg);
std::vector<torch::Tensor> gauss_head_fwd(torch::Tensor hin, torch::Tensor Wm,
                                          torch::Tensor bm, torch::Tensor Wl,
                                          torch::Tensor bl, torch::Tensor eps,
                                          c10::optional<torch::Tensor> Ws_c,
                                          c10::optional<torch::Tensor> bs_c);
torch::Tensor gauss_head_bwd(
    c10::optional<torch::Tensor> dz, c10::optional<torch::Tensor> dmu,
    c10::optional<torch::Tensor> dlv, torch::Tensor eps, torch::Tensor lv,
    torch::Tensor hin, torch::Tensor Ws, long N_,
    c10::optional<torch::Tensor> dWm, c10::optional<torch::Tensor> dbm,
    c10::optional<torch::Tensor> dWl, c10::optional<torch::Tensor> dbl);
torch::Tensor tanh_head_fwd(torch::Tensor hin, torch::Tensor W,
                            torch::Tensor b);
torch::Tensor tanh_head_bwd(torch::Tensor dy, torch::Tensor y,
                            torch::Tensor hin, torch::Tensor W,
                            c10::optional<torch::Tensor> dW_acc,
                            c10::optional<torch::Tensor> db_acc);
torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor B);
torch::Tensor tr16_probe(long mode);
std::vector<torch::Tensor> conv2d_nhwc_fwd(torch::Tensor in, torch::Tensor w,
                                            c10::optional<torch::Tensor> bias,
                                            long stride, long pad, long act,
                                            bool want_stats, long oh, long ow,
                                            long oy0, long ox0);
std::vector<torch::Tensor> conv2d_nhwc_fracstride(
    torch::Tensor in, torch::Tensor w, c10::optional<torch::Tensor> bias,
    long up_stride, long up_pad, long OH, long OW, long act, bool want_stats,
    long in_ring, long out_ring);
std::vector<torch::Tensor> conv2d_glds_fwd(
    torch::Tensor in, torch::Tensor w, c10::optional<torch::Tensor> bias,
    long stride, long act, bool want_stats, long oh, long ow, long oy0,
    long ox0, c10::optional<torch::Tensor> in2,
    c10::optional<torch::Tensor> out2_k1);
std::vector<torch::Tensor> bn_act_fwd_train(
    torch::Tensor x, torch::Tensor stats, torch::Tensor gamma,
    torch::Tensor beta, c10::optional<torch::Tensor> running_mean,
    c10::optional<torch::Tensor> running_var, double momentum, double eps,
    long act, long ring);
torch::Tensor bn_act_fwd_eval(torch::Tensor x, torch::Tensor gamma,
                              torch::Tensor beta, torch::Tensor running_mean,
                              torch::Tensor running_var, double eps, long act,
                              long ring);
std::vector<torch::Tensor> bn_act_bwd(torch::Tensor x, torch::Tensor dy,
                                      torch::Tensor mean, torch::Tensor invstd,
                                      torch::Tensor gamma, torch::Tensor beta,
                                      torch::Tensor scale, long act,
                                      c10::optional<torch::Tensor> dgamma_acc,
                                      c10::optional<torch::Tensor> dbeta_acc,
                                      long ring);
torch::Tensor conv2d_nhwc_wgrad(torch::Tensor Y, torch::Tensor X, long R,
                                long S, long stride, long pad, long splitp,
                                c10::optional<torch::Tensor> acc, long yring,
                                c10::optional<torch::Tensor> X2, long thin,
                                long taps);
std::string conv2d_wgrad_path(long B, long A, long A1, long HO, long WO,
                              long yring, long taps);
void set_wgrad_rows(bool on);
bool wgrad_rows();
void set_wgrad_narrow(bool on);
bool wgrad_narrow();
std::vector<torch::Tensor> maxpool2x2_fwd(torch::Tensor in, long ri, long ro);
torch::Tensor maxpool2x2_bwd(torch::Tensor gout, torch::Tensor idx, long H,
                             long W, long ri, long ro);
torch::Tensor upsample2x_fwd(torch::Tensor in, long ri, long ro);
torch::Tensor upsample2x_bwd(torch::Tensor gout, long ri, long ro);
torch::Tensor channel_sum_nhwc(torch::Tensor x,
                               c10::optional<torch::Tensor> acc);
void set_bn_tail_fused(bool fused);
bool bn_tail_fused();
torch::Tensor sqdiff_sum(torch::Tensor a, torch::Tensor b);
torch::Tensor moving_mnist_render(torch::Tensor digits, torch::Tensor idx,
                                  torch::Tensor pos, long S);
std::vector<torch::Tensor> frame_metrics(torch::Tensor a, torch::Tensor b,
                                         torch::Tensor win, double data_range);
torch::Tensor clip_gather(torch::Tensor bank, torch::Tensor idx, long L);
std::vector<torch::Tensor> pose_metrics(torch::Tensor gen, torch::Tensor ref,
                                        double w0, double w1, double w2);
torch::Tensor pose_spread(torch::Tensor gen, double w0, double w1, double w2);
long pose_spread_max_sj();

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("mfma_probe", &mfma_probe, "16x16x32 bf16 MFMA layout probe");
  m.def("affine4_fwd", &affine4_fwd, "concat-free 4-source affine (gfx950)");
  m.def("affine4_bwd", &affine4_bwd, "affine4 backward (managed dW/db)");
  m.def("gauss_head_fwd", &gauss_head_fwd,
        "fused mu/logvar/reparameterize head (gfx950)");
  m.def("gauss_head_bwd", &gauss_head_bwd, "gauss head backward");
  m.def("tanh_head_fwd", &tanh_head_fwd, "fused Linear+Tanh head (gfx950)");
  m.def("tanh_head_bwd", &tanh_head_bwd, "tanh head backward");
  m.def("tr16_probe", &tr16_probe, "ds_read_b64_tr_b16 semantics probe");
  m.def("conv2d_nhwc_fwd", &conv2d_nhwc_fwd,
        "NHWC implicit-GEMM bf16 conv fwd (gfx950 MFMA); returns (out, stats)",
        pybind11::arg("in"), pybind11::arg("w"), pybind11::arg("bias"),
        pybind11::arg("stride"), pybind11::arg("pad"), pybind11::arg("act"),
        pybind11::arg("want_stats") = false, pybind11::arg("oh") = 0,
        pybind11::arg("ow") = 0, pybind11::arg("oy0") = 0,
        pybind11::arg("ox0") = 0);
  m.def("conv2d_nhwc_fracstride", &conv2d_nhwc_fracstride,
        "fractionally-strided conv, in-kernel parity loop (ConvT fwd / s2 dgrad)",
        pybind11::arg("in"), pybind11::arg("w"), pybind11::arg("bias"),
        pybind11::arg("up_stride"), pybind11::arg("up_pad"), pybind11::arg("OH"),
        pybind11::arg("OW"), pybind11::arg("act"),
        pybind11::arg("want_stats") = false, pybind11::arg("in_ring") = 0,
        pybind11::arg("out_ring") = 0);
  m.def("conv2d_glds_fwd", &conv2d_glds_fwd,
        "NHWC conv fwd, glds 3-buffer pipeline (padded-input contract)",
        pybind11::arg("in"), pybind11::arg("w"), pybind11::arg("bias"),
        pybind11::arg("stride"), pybind11::arg("act"),
        pybind11::arg("want_stats") = false, pybind11::arg("oh") = 0,
        pybind11::arg("ow") = 0, pybind11::arg("oy0") = 0,
        pybind11::arg("ox0") = 0, pybind11::arg("in2") = c10::nullopt,
        pybind11::arg("out2") = c10::nullopt);
  m.def("bn_act_fwd_train", &bn_act_fwd_train, "fused BN+act train fwd (gfx950)",
        pybind11::arg("x"), pybind11::arg("stats"), pybind11::arg("gamma"),
        pybind11::arg("beta"), pybind11::arg("running_mean"),
        pybind11::arg("running_var"), pybind11::arg("momentum"),
        pybind11::arg("eps"), pybind11::arg("act"),
        pybind11::arg("ring") = 0);
  m.def("bn_act_fwd_eval", &bn_act_fwd_eval, "fused BN+act eval fwd (gfx950)",
        pybind11::arg("x"), pybind11::arg("gamma"), pybind11::arg("beta"),
        pybind11::arg("running_mean"), pybind11::arg("running_var"),
        pybind11::arg("eps"), pybind11::arg("act"), pybind11::arg("ring") = 0);
  m.def("bn_act_bwd", &bn_act_bwd, "fused BN+act bwd (gfx950, deterministic)",
        pybind11::arg("x"), pybind11::arg("dy"), pybind11::arg("mean"),
        pybind11::arg("invstd"), pybind11::arg("gamma"), pybind11::arg("beta"),
        pybind11::arg("scale"), pybind11::arg("act"),
        pybind11::arg("dgamma_acc") = c10::nullopt,
        pybind11::arg("dbeta_acc") = c10::nullopt,
        pybind11::arg("ring") = 0);
  m.def("channel_sum_nhwc", &channel_sum_nhwc,
        "NHWC per-channel sum, fp32 out (gfx950, deterministic)",
        pybind11::arg("x"), pybind11::arg("acc") = c10::nullopt);
  m.def("set_bn_tail_fused", &set_bn_tail_fused,
        "BN statistics tail: true = one fused launch (default), false = the "
        "split fold/finalize/combine launches (bitwise the same results)",
        pybind11::arg("fused"));
  m.def("bn_tail_fused", &bn_tail_fused, "current BN statistics tail mode");
  m.def("conv2d_nhwc_wgrad", &conv2d_nhwc_wgrad,
        "NHWC wgrad, split-K over pixel slabs (gfx950 MFMA, deterministic); "
        "acc: fp32 dense (B,R,S,A)-layout tensor to accumulate into; "
        "thin: -1 auto, 0 never, 1 require the thin-channel path; "
        "taps: the same for the single-pass all-taps 3x3 strip kernel, 2 "
        "requires the row-order all-taps kernel (3 / 4: 64x64 / 32x64 "
        "tiles), 5 the narrow all-taps kernel (16-wide maps; 6 / 7: 64x64 / "
        "128x64 tiles)",
        pybind11::arg("Y"), pybind11::arg("X"), pybind11::arg("R"),
        pybind11::arg("S"), pybind11::arg("stride"), pybind11::arg("pad"),
        pybind11::arg("splitp") = 0, pybind11::arg("acc") = c10::nullopt,
        pybind11::arg("yring") = 0, pybind11::arg("X2") = c10::nullopt,
        pybind11::arg("thin") = -1, pybind11::arg("taps") = -1);
  m.def("conv2d_wgrad_path", &conv2d_wgrad_path,
        "host only: path of a 3x3 s1 pad-0 ringed-X wgrad call: 'per_tap', "
        "'taps_strip', 'taps_rows' or 'taps_narrow'",
        pybind11::arg("B"), pybind11::arg("A"), pybind11::arg("A1"),
        pybind11::arg("HO"), pybind11::arg("WO"), pybind11::arg("yring"),
        pybind11::arg("taps") = -1);
  m.def("set_wgrad_rows", &set_wgrad_rows,
        "auto may use the row-order all-taps wgrad kernel (default true); "
        "false keeps those classes on the per-tap path (bitwise the same)",
        pybind11::arg("on"));
  m.def("wgrad_rows", &wgrad_rows, "current row-order wgrad auto mode");
  m.def("set_wgrad_narrow", &set_wgrad_narrow,
        "auto may use the narrow all-taps wgrad kernel on 16-wide maps "
        "(default true); false keeps those classes on the per-tap path "
        "(bitwise the same)",
        pybind11::arg("on"));
  m.def("wgrad_narrow", &wgrad_narrow, "current narrow wgrad auto mode");
  m.def("maxpool2x2_fwd", &maxpool2x2_fwd, "NHWC 2x2/s2 maxpool fwd (gfx950)",
        pybind11::arg("in"), pybind11::arg("ri") = 0, pybind11::arg("ro") = 0);
  m.def("maxpool2x2_bwd", &maxpool2x2_bwd, "NHWC 2x2/s2 maxpool bwd (gfx950)",
        pybind11::arg("gout"), pybind11::arg("idx"), pybind11::arg("H"),
        pybind11::arg("W"), pybind11::arg("ri") = 0, pybind11::arg("ro") = 0);
  m.def("upsample2x_fwd", &upsample2x_fwd, "NHWC nearest x2 fwd (gfx950)",
        pybind11::arg("in"), pybind11::arg("ri") = 0, pybind11::arg("ro") = 0);
  m.def("upsample2x_bwd", &upsample2x_bwd, "NHWC nearest x2 bwd (gfx950)",
        pybind11::arg("gout"), pybind11::arg("ri") = 0, pybind11::arg("ro") = 0);
  m.def("lstm_cell_fwd", &lstm_cell_fwd, "fused LSTM cell forward (gfx950)");
  m.def("lstm_cell_bwd_pointwise", &lstm_cell_bwd_pointwise,
        "LSTM cell backward pointwise (gfx950)");
  m.def("multi_tensor_adam", &multi_tensor_adam, "multi-tensor Adam (gfx950)");
  m.def("gaussian_kl_fwd", &gaussian_kl_fwd, "fused gaussian KL fwd (gfx950)");
  m.def("gaussian_kl_bwd", &gaussian_kl_bwd, "fused gaussian KL bwd (gfx950)");
  m.def("sqdiff_sum", &sqdiff_sum, "fused sum((a-b)^2), bf16/f32 in fp32 out");
  m.def("moving_mnist_render", &moving_mnist_render,
        "MovingMNIST frames from a host-validated trajectory plan (gfx950); "
        "digits (N,32,32) f32, idx (B,D) i32, pos (L,B,D,2) i32 -> "
        "(L,B,1,S,S) f32",
        pybind11::arg("digits"), pybind11::arg("idx"), pybind11::arg("pos"),
        pybind11::arg("S"));
  m.def("frame_metrics", &frame_metrics,
        "fused per-image SSIM + MSE (gfx950, deterministic); a, b (M,C,H,W) "
        "strided fp32/bf16/fp16, win = eleven fp32 window weights on the CPU "
        "-> (ssim (M) f32, mse (M) f32)",
        pybind11::arg("a"), pybind11::arg("b"), pybind11::arg("win"),
        pybind11::arg("data_range") = 1.0);
  m.def("clip_gather", &clip_gather,
        "batch gather from a uint8 frame bank (gfx950); bank (N,T,H,W,C) u8, "
        "idx (B) i32 host-validated -> (L,B,H,W,C) f32 = bank[idx, :L] / 255, "
        "correctly rounded",
        pybind11::arg("bank"), pybind11::arg("idx"), pybind11::arg("L"));
  m.def("pose_metrics", &pose_metrics,
        "per-frame MPJPE + MSE of S pose samples (gfx950, deterministic); gen "
        "(T,S,B,J,3), ref (T,B,J,3) contiguous fp32/bf16/fp16, w = per-axis "
        "scales -> (mpjpe (S,T,B) f32, mse (S,T,B) f32)",
        pybind11::arg("gen"), pybind11::arg("ref"), pybind11::arg("w0"),
        pybind11::arg("w1"), pybind11::arg("w2"));
  m.def("pose_spread", &pose_spread,
        "mean pairwise per-joint distance between the S samples of a frame "
        "(gfx950, deterministic); gen (T,S,B,J,3) contiguous fp32/bf16/fp16, "
        "S >= 2, S * J <= pose_spread_max_sj() -> (T,B) f32",
        pybind11::arg("gen"), pybind11::arg("w0"), pybind11::arg("w1"),
        pybind11::arg("w2"));
  m.def("pose_spread_max_sj", &pose_spread_max_sj,
        "host only: the largest S * J pose_spread stages in LDS");
}
