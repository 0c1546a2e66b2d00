// conv3x3_engine.h -- which engine the convolution operators run a 3x3 / stride 1 / pad 1 fp32 problem on.
//
// The one statement of the operator surface's rule (Conv, ConvGradient, ConvGroup, ConvGradientGroup and
// c2hip_conv3x3_engine all call it; the native pipelines have their own in engines.py).  Like cuDNN's
// internal choice (conv_op_cudnn.cc:541-558) it goes by the width of the output: the forward pass asks with its M
// output channels, the data gradient -- the forward kernel on the flipped / transposed pack -- with its C.
//
//   hip_algo   "auto" (default, and any string not listed here): F(2x2, 3x3) Winograd from 32 outputs up, else direct
//              "direct" | "winograd"   pin the engine
//              "winograd24"            F(2x4, 3x3) from 128 outputs up, the automatic choice below
//              "split"                 the split-operand engine from 256 outputs up, F(2x4) from 128, automatic below;
//                                      and the filter gradient on the split-operand engine from 128 x 64 up
//   ("winograd24" and "split" are what the net lowering assigns, ops/net_lowering.cc)
#ifndef C2HIP_CONV3X3_ENGINE_H_
#define C2HIP_CONV3X3_ENGINE_H_

#include <string>

namespace caffe2 {

enum class Conv3x3Engine { DIRECT, WINO, WINO24, SPLIT };

inline Conv3x3Engine PickConv3x3Engine(const std::string& algo, int out_channels) {
  if (algo == "direct") return Conv3x3Engine::DIRECT;
  if (algo == "winograd") return Conv3x3Engine::WINO;
  if (algo == "split" && out_channels >= 256) return Conv3x3Engine::SPLIT;
  if ((algo == "split" || algo == "winograd24") && out_channels >= 128) return Conv3x3Engine::WINO24;
  return out_channels >= 32 ? Conv3x3Engine::WINO : Conv3x3Engine::DIRECT;
}

// the filter gradient [M][C][3][3] on the split-operand engine (conv3x3_wgrad_split.hip) instead of the fp32 one
inline bool SplitFilterGradient(const std::string& algo, int M, int C) {
  return algo == "split" && M >= 128 && C >= 64;
}

}  // namespace caffe2
#endif  // C2HIP_CONV3X3_ENGINE_H_
