// Prints what csrc/conv_rules.h says about a grid of convolutions, one line per point, for tests/test_conv_rules_host.py to
// hold packer.py's pure-Python predicates against.  No GPU, no HIP:
//   c++ -std=c++17 -O1 tools/conv_rules_check.cpp -o conv_rules_check  &&  ./conv_rules_check
// Per line: ks stride cin cout H W | conv_n_tiles takes_wino3 takes_wino24b takes_wino24c takes_pp2 takes_x3 takes_x3p
// takes_x3s2 takes_p1 takes_dma | conv_algo_reject == nullptr for algos 0..7 | conv_weight_floats for algos 0..7.
// One group, channel strides rounded up to 4, offsets 0, no residual, fp32.
#include "../arbitrary-hands-3d-reconstruction_amd/csrc/conv_rules.h"

#include <cstdio>

using namespace acrmi;

int main() {
  const int kss[] = {1, 3}, strides[] = {1, 2};
  const int cins[] = {8, 16, 24, 32, 34, 48, 64, 96, 128}, couts[] = {16, 32, 33, 40, 64, 96, 128};
  const int sizes[] = {8, 15, 16, 24, 31, 32, 48, 63, 64};
  for (int ks : kss)
    for (int stride : strides)
      for (int cin : cins)
        for (int cout : couts)
          for (int H : sizes)
            for (int W : sizes) {
              ConvShape s{};
              s.ks = ks; s.stride = stride; s.groups = 1; s.cin = cin; s.cout = cout;
              s.H = H; s.W = W; s.Ho = conv_out_size(H, ks, stride); s.Wo = conv_out_size(W, ks, stride);
              s.in_cs = (cin + 3) / 4 * 4; s.out_cs = (cout + 3) / 4 * 4;
              std::printf("%d %d %d %d %d %d | %d %d %d %d %d %d %d %d %d %d |", ks, stride, cin, cout, H, W, conv_n_tiles(cout),
                          (int)takes_wino3(s), takes_wino24b(s), (int)takes_wino24c(s), (int)takes_pp2(s), takes_x3(s),
                          (int)takes_x3p(s), (int)takes_x3s2(s), (int)takes_p1(s), (int)takes_dma(s));
              for (int algo = 0; algo < 8; ++algo) std::printf(" %d", (int)(conv_algo_reject(algo, s) == nullptr));
              std::printf(" |");
              for (int algo = 0; algo < 8; ++algo) std::printf(" %lld", conv_weight_floats(algo, 1, ks, cin, cout, 0));
              std::printf("\n");
            }
  return 0;
}
