// Which convolution kernel takes which layer: the ONE statement of the shape rules.  Read by the launchers (conv_mfma.hip,
// conv_*.inc), by the validators of the C ABI (acrmi_conv2d*, acrmi_set_program) and, through tools/conv_rules_check.cpp and
// tests/test_conv_rules_host.py, held against packer.py's pure-Python copies.  Plain C++17, host only, no HIP header.
// Forced tuning cfgs, experiment_env switches and the CU-count heuristics are no shape rules: they stay in the launchers.
#pragma once

namespace acrmi {

// A convolution as the rules see it (strides, offsets and channel counts in elements of their tensor; cin, cout per group).
struct ConvShape {
  int ks, stride, groups, cin, cout, H, W, Ho, Wo;
  int in_cs, in_coff, out_cs, out_coff, res_cs, res_coff, out2_cs, out2_coff;
  int has_res;            // a residual (or, res_bcast, a position-bias map) is added
  int bias_fstride;       // floats between the frames' bias rows (0 = one row for all)
  int nxt, out2;          // extra residual terms (ConvArgs::xt); a second output (ConvArgs::out2)
  int splitk, res_bcast, in_sub;
  int dtype, out_f32;     // ACRMI_DT_* of the input; 16-bit input with fp32 output and residual
};

// ---- geometry ----------------------------------------------------------------------------------------------------------
constexpr int conv_out_size(int in, int ks, int stride) { return (in + 2 * (ks / 2) - ks) / stride + 1; }      // padding ks / 2
// 32-cout tiles per group in the packed weights and bias: whole 64-cout blocks above 32 channels
constexpr int conv_n_tiles(int cout) { return cout <= 32 ? 1 : ((cout + 63) / 64) * 2; }
// steps of one tap = 1 KiB weight fragments per tap and n-tile: 8 input channels each (16-bit storage: 16)
constexpr int conv_ksteps(int cin, int dtype) { return dtype ? (cin + 15) / 16 : (cin + 7) / 8; }
// taps of the packed weights: F(2,3) along x 3x4, F(2x2,3x3) 4x4, F(2x4,3x3) 4x6, polyphase 4x7, else the filter's own
constexpr int conv_taps(int algo, int ks) { return algo >= 6 ? ks * ks : algo == 5 ? 28 : algo == 4 ? 24 : algo >= 2 ? 16 : algo == 1 ? 12 : ks * ks; }
// floats of an op's packed weights (algo 3: the LDS image of conv_wino3_kernel; algo 6 / 7: + the weight scale)
constexpr long long conv_weight_floats(int algo, int groups, int ks, int cin, int cout, int dtype) {
  return algo == 3 ? 16384 : (long long)groups * conv_taps(algo, ks) * conv_ksteps(cin, dtype) * conv_n_tiles(cout) * 256 + (algo >= 6);
}

// ---- clauses the kernels share ---------------------------------------------------------------------------------------------
inline bool conv_in_aligned(const ConvShape& s) { return s.in_cs % 4 == 0 && s.in_coff % 4 == 0; }
inline bool conv_out_aligned(const ConvShape& s) { return s.out_cs % 4 == 0 && s.out_coff % 4 == 0; }
inline bool conv_res_aligned(const ConvShape& s) { return !s.has_res || (s.res_cs % 4 == 0 && s.res_coff % 4 == 0); }
inline bool conv_c32(const ConvShape& s) { return s.cin % 32 == 0 && s.cin >= 32 && s.cout % 32 == 0; }
inline bool conv_same_map(const ConvShape& s) { return s.H == s.Ho && s.W == s.Wo; }
// The four-wave frame: 16-byte aligned channel slices, no split-K, a dense input, a patch (halo_rows x W pixels; the 1x1
// kernels: halo_rows = 0, their 256 pixels) inside one buffer descriptor, a per-frame bias row that holds every packed n-tile.
inline bool conv_frame4(const ConvShape& s, int halo_rows) {
  return conv_in_aligned(s) && conv_out_aligned(s) && conv_res_aligned(s) && !s.splitk && s.in_sub <= 1 &&
         (halo_rows ? (long long)halo_rows * s.W : 256) * s.in_cs * 4 < (1ll << 30) &&
         (s.bias_fstride == 0 || s.bias_fstride >= s.groups * conv_n_tiles(s.cout) * 32);
}

// ---- one predicate per kernel ------------------------------------------------------------------------------------------------
inline bool takes_wino3(const ConvShape& s) {      // algo 3: Cin <= 32, Cout = 32, the layer's taps resident in LDS
  return s.ks == 3 && s.stride == 1 && s.groups == 1 && s.cin <= 32 && s.cout == 32 && s.bias_fstride == 0 && s.Ho % 8 == 0 &&
         s.Wo % 16 == 0 && conv_out_aligned(s) && conv_in_aligned(s) && conv_res_aligned(s);
}
// algo 4 (what it does not take stays on conv_wino24_kernel).  Item width: 32 (8x32 pixels), 16 (16x16 pixels, maps narrower
// than 32 pixels) or 0; n-tiles per wave: 2 when Cout % 64 == 0, else 1 (8x32-pixel items only)
inline int takes_wino24b(const ConvShape& s) {
  if (!(s.ks == 3 && s.stride == 1 && conv_c32(s) && conv_same_map(s) && conv_frame4(s, 10))) return 0;
  if (s.Ho % 8 == 0 && s.Wo % 32 == 0) return 32;
  return (s.Ho % 16 == 0 && s.Wo % 16 == 0 && s.cout % 64 == 0 && s.cin >= 64) ? 16 : 0;
}
inline bool takes_wino24c(const ConvShape& s) { return takes_wino24b(s) == 32 && s.cin >= 64 && s.cout % 64 == 0; }      // algo 4 under cfg 842
inline bool takes_pp2(const ConvShape& s) {      // algo 5
  return s.ks == 3 && s.stride == 2 && s.H % 2 == 0 && s.W % 2 == 0 && s.Ho == s.H / 2 && s.Wo == s.W / 2 && s.Ho % 8 == 0 &&
         s.Wo % 16 == 0 && s.cin % 16 == 0 && s.cout % 32 == 0 && conv_frame4(s, 17);
}
inline int takes_x3(const ConvShape& s) {      // algo 6 / 7, 3x3 stride 1: 32 (8x32-pixel items), 16 (16x16) or 0
  if (!(s.ks == 3 && s.stride == 1 && conv_c32(s) && conv_same_map(s) && conv_frame4(s, 18))) return 0;
  return (s.Ho % 8 == 0 && s.Wo % 32 == 0) ? 32 : (s.Ho % 16 == 0 && s.Wo % 16 == 0) ? 16 : 0;
}
inline bool takes_x3s2(const ConvShape& s) {      // algo 6 / 7, 3x3 stride 2
  return s.ks == 3 && s.stride == 2 && conv_c32(s) && s.H == 2 * s.Ho && s.W == 2 * s.Wo && s.Ho % 8 == 0 && s.Wo % 32 == 0 &&
         s.nxt == 0 && conv_frame4(s, 34);
}
inline bool takes_p1(const ConvShape& s) {      // algo 0, 1x1 stride 1 (where launch_conv's item count says so): 256-pixel items
  return s.ks == 1 && s.stride == 1 && conv_c32(s) && conv_same_map(s) && (s.Ho * s.Wo) % 256 == 0 && conv_frame4(s, 0);
}
inline bool takes_x3p(const ConvShape& s) { return takes_p1(s); }      // algo 6 / 7, 1x1: the same items
inline bool takes_dma(const ConvShape& s) { return s.cin % 4 == 0 && conv_in_aligned(s); }      // LDS-DMA loaders: whole channel quads

// ---- does launch_conv have a kernel for this algo and shape?  null = yes, else the sentence for the error message ---------------
inline const char* conv_algo_reject(int algo, const ConvShape& s) {
  if (algo < 0 || algo > 7) return "unknown conv algo (0..7)";
  if ((s.ks != 1 && s.ks != 3) || (s.stride != 1 && s.stride != 2)) return "only 3x3 and 1x1 convolutions at stride 1 / 2 are implemented";
  if (s.nxt < 0 || s.nxt > 3) return "at most 3 extra residual terms";
  if (s.dtype) {      // f16 / bf16 storage (conv_h16.hip): 8 elements per 16-byte vector
    if (algo != 0 || s.splitk || s.nxt || s.out2 || s.res_bcast)
      return "16-bit storage runs the direct kernels only: algo 0, no split-K, extra residual terms, second output or bias map";
    if (s.out_f32 && s.stride != 1) return "16-bit input with fp32 output exists at stride 1 only";
    const int oq = s.out_f32 ? 4 : 8;
    return (s.in_cs % 8 || s.in_coff % 8 || (s.groups > 1 && s.cin % 8) || s.out_cs % oq || (s.has_res && s.res_cs % oq))
               ? "16-bit storage: channel strides, the input offset and a group's first channel must be multiples of 16 bytes" : nullptr;
  }
  if (!conv_in_aligned(s) || (s.groups > 1 && s.cin % 4)) return "in_cs, in_coff and a group's first channel must be multiples of 4";
  if (s.splitk && (algo != 2 || s.groups < 2 || s.groups > 8 || s.cin % 32 || s.cin < 64 || s.cout == 33 || s.bias_fstride))
    return "split-K needs algo 2, 2..8 slices of Cin % 32 == 0, Cin >= 64 channels each, Cout != 33, no per-frame bias";
  if (s.nxt > 0 && algo != 5 && algo != 0 && !(algo == 3 && s.out2))
    return "extra residual terms need a 3x3 stride-2 convolution (algo 0 / 5) or the second output of algo 3";
  if (s.out2 && algo != 3) return "a second output needs algo 3";
  if (s.res_bcast && algo == 3) return "a position-bias map needs an algo other than 3";
  // a kernel of the four-wave frame refuses: for the frame's own clause, or for the kernel's geometry
  auto why = [&](int halo_rows, const char* geometry) {
    return conv_frame4(s, halo_rows) ? geometry : "the four-wave frame needs in_cs, in_coff, out_cs, out_coff, res_cs, res_coff % 4 == 0, a per-frame "
                                                  "bias row of groups * n_tiles * 32 floats, a halo patch below 2^30 bytes";
  };
  const bool s11 = s.ks == 3 && s.stride == 1;
  if (algo >= 6 && s.ks == 1) return takes_x3p(s) ? nullptr : why(0, "algo 6 / 7 (1x1) needs stride 1, Cin % 32 == 0, Cout % 32 == 0, a map of whole 256-pixel items");
  if (algo >= 6 && s.stride == 2)
    return takes_x3s2(s) ? nullptr : why(34, "algo 6 / 7 at stride 2 needs Cin % 32 == 0, Cout % 32 == 0, an even input size (H = 2 Ho, W = 2 Wo), an output map of "
                                             "8x32-pixel tiles, no extra residual terms");
  if (algo >= 6) return takes_x3(s) ? nullptr : why(18, "algo 6 / 7 (3x3 stride 1) needs Cin % 32 == 0, Cout % 32 == 0, a map of 8x32- or 16x16-pixel tiles");
  if (algo == 5) return takes_pp2(s) ? nullptr : why(17, "algo 5 needs a 3x3 stride-2 convolution, Cin % 16 == 0, Cout % 32 == 0, an even input size, an output map of 8x16-pixel tiles");
  if (algo == 4)      // conv_wino24b_kernel where it applies, else conv_wino24_kernel: two 32-channel chunks per item
    return (s11 && (takes_wino24b(s) || conv_ksteps(s.cin, 0) * 8 > 32)) ? nullptr
           : "algo 4 needs a 3x3 stride-1 convolution with Cin > 32 - or Cin = 32 with Cout % 32 == 0 on a map of 8x32-pixel tiles, 16-byte aligned channel slices";
  if (algo == 3 && !takes_wino3(s))
    return "algo 3 needs a 3x3 stride-1 convolution, groups 1, Cin <= 32, Cout = 32, no per-frame bias, a map of 8x16-pixel tiles, out_cs, out_coff, res_cs, res_coff % 4 == 0";
  if (algo == 3 && s.out2 && (!takes_dma(s) || s.nxt < 1 || s.out2_cs % 4 || s.out2_coff % 4))
    return "the second output of algo 3 needs Cin % 4 == 0, 1..3 extra residual terms, out2_cs, out2_coff % 4 == 0";
  if ((algo == 1 || algo == 2) && !s11) return "algo 1 / 2 needs a 3x3 stride-1 convolution";
  if (algo == 0 && s.nxt > 0 && (s.ks != 3 || s.stride != 2 || conv_ksteps(s.cin, 0) * 8 <= 16 || s.cout % 32 || !conv_out_aligned(s)))
    return "extra residual terms on algo 0 need a 3x3 stride-2 convolution with Cin > 16, Cout % 32 == 0, out_cs, out_coff % 4 == 0";
  return nullptr;
}

}  // namespace acrmi
