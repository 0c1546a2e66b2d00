// Conv / ConvGradient for HIPContext.
//
// Argument handling follows ConvPoolOpBase (caffe2/operators/
// conv_pool_op_base.h:45-194): `kernel` | `kernel_h`+`kernel_w` | `kernels`,
// likewise stride(s), pad(s) / pad_t..pad_r, dilation(s), `group`, `order`,
// `legacy_pad`.  Inputs/outputs follow conv_op.h:29-91 and
// conv_gradient_op.cc:35-77: Conv [X, filter, (bias)] -> [Y];
// ConvGradient [X, filter, dY] -> [dfilter, dbias, (dX)] or, with
// no_bias=1, [dfilter, (dX)].
//
// Two engines, chosen per definition like the reference's engine fall-through
// (caffe2/core/operator.cc:116-200): the geometry the RetinaNet subnets and the
// ResNet bottlenecks use (3x3, stride 1, pad 1, dilation 1, group 1, NCHW) runs on
// the matrix-core kernels of this repo; every other 2-D NCHW geometry (the
// backbone's 1x1, strided and 7x7 layers, and `group` > 1 -- ResNeXt's grouped 3x3 --
// as one strided-batched GEMM per image) runs on the DEFAULT engine of
// conv_op_impl.h:31-202 / :358-577 -- im2col + GEMM per image, with the GEMMs on this
// repo's general fp32-MFMA kernel (kernels/gemm_general.hip; no vendor BLAS).  NHWC and non-2-D convolutions raise UnsupportedOperatorFeature at
// construction (caffe2/core/operator.h:765-782).  The 3x3 engines' packed filter is
// cached per operator and rebuilt only when the filter blob was written since the last Run
// (ops/filter_pack_cache.h: Tensor::version()) -- round 5; rounds 1-4 repacked on every Run.
//
// float16 blobs (TensorProto::FLOAT16) dispatch like CudnnConvOp's DoRunWithType<float16, ...>
// (conv_op_cudnn.cc:631-636, :1115-1124): fp16 storage for X, filter, bias, Y and all
// gradients, fp32 math -- on the fp16 matrix-core kernels of kernels/conv3x3_f16.hip, for the
// 3x3 / stride 1 / pad 1 geometry.
//
// Two optional arguments exist for graph-level fusion and are NOT emitted by
// the reference graph builder (absent = reference behaviour):
//   Conv          fuse_relu=1             Y = max(conv, 0)  (Conv + in-place Relu)
//   Conv          fuse_sigmoid=1          Y = 1 / (1 + exp(-conv))  (Conv + Sigmoid; the 3x3 fp32 engines)
//   ConvGradient  relu_grad_on_input=1    dX masked by X > 0 (= ReluGradient of
//                                         the in-place Relu that produced X)
//   both          hip_algo                which 3x3 engine: the rule and its strings are in ops/conv3x3_engine.h
//   both          hip_algo="grouped"      opt-in: a grouped 3x3 / pad 1 / stride 1|2 layer with 4, 8, 16, 32 or 64
//                                         channels per group (ResNeXt) on kernels/grouped_conv3x3{,_grad}.hip instead
//                                         of the default engine; any other geometry fails by name (no fall-back)
#ifndef C2HIP_CONV_OP_H_
#define C2HIP_CONV_OP_H_

#include <atomic>

#include "c2/operator.h"
#include "ops/filter_pack_cache.h"

namespace caffe2 {

// process-wide counters behind c2hip_counter() (tests: the pack cache and the net lowering at work)
extern std::atomic<long long> g_filter_packs_issued;
extern std::atomic<long long> g_conv_launch_calls;

struct ConvGeometry {
  vector<int> kernel, stride, pads, dilation;
  int group = 1;
  string order = "NCHW";
};

// The argument accessors of OperatorBase over a bare definition: lets the net lowering
// (ops/net_lowering.cc) read a convolution's geometry before any operator exists.
class DefArgs {
 public:
  explicit DefArgs(const OperatorDef& def) {
    for (const Argument& a : def.arg) args_[a.name] = &a;
  }
  bool HasArgument(const string& n) const { return args_.count(n) != 0; }
  template <typename T> T GetSingleArgument(const string& n, const T& dflt) const;
  template <typename T> vector<T> GetRepeatedArgument(const string& n, const vector<T>& dflt = {}) const;

 private:
  std::map<string, const Argument*> args_;
};
template <> inline int DefArgs::GetSingleArgument<int>(const string& n, const int& d) const {
  auto it = args_.find(n);
  if (it == args_.end()) return d;
  CAFFE_ENFORCE(it->second->has_i, "Argument ", n, " does not have an integer value");
  return (int)it->second->i;
}
template <> inline string DefArgs::GetSingleArgument<string>(const string& n, const string& d) const {
  auto it = args_.find(n);
  if (it == args_.end()) return d;
  CAFFE_ENFORCE(it->second->has_s, "Argument ", n, " does not have a string value");
  return it->second->s;
}
template <> inline vector<int> DefArgs::GetRepeatedArgument<int>(const string& n, const vector<int>& d) const {
  auto it = args_.find(n);
  if (it == args_.end()) return d;
  return vector<int>(it->second->ints.begin(), it->second->ints.end());
}

// caffe2/operators/conv_pool_op_base.h:45-194, restated.
template <class ArgSource>
ConvGeometry ParseConvGeometryFrom(const ArgSource& op) {
  ConvGeometry g;
  g.kernel = op.template GetRepeatedArgument<int>("kernels");
  g.stride = op.template GetRepeatedArgument<int>("strides");
  g.pads = op.template GetRepeatedArgument<int>("pads");
  g.dilation = op.template GetRepeatedArgument<int>("dilations");
  g.group = op.template GetSingleArgument<int>("group", 1);
  g.order = op.template GetSingleArgument<string>("order", "NCHW");
  const int legacy_pad = op.template GetSingleArgument<int>("legacy_pad", 0);   // NOTSET
  CAFFE_ENFORCE(legacy_pad == 0 || legacy_pad == 3,
                "legacy padding VALID/SAME is not supported by the HIP conv operators");

  auto pair_arg = [&](const char* single, const char* h, const char* w, vector<int>* out) {
    if (op.HasArgument(single)) {
      out->assign(2, op.template GetSingleArgument<int>(single, 0));
    } else if (op.HasArgument(h) && op.HasArgument(w)) {
      out->push_back(op.template GetSingleArgument<int>(h, 0));
      out->push_back(op.template GetSingleArgument<int>(w, 0));
    }
  };
  pair_arg("kernel", "kernel_h", "kernel_w", &g.kernel);
  pair_arg("stride", "stride_h", "stride_w", &g.stride);
  pair_arg("dilation", "dilation_h", "dilation_w", &g.dilation);
  if (op.HasArgument("pad")) {
    g.pads.assign(4, op.template GetSingleArgument<int>("pad", 0));
  } else if (op.HasArgument("pad_t") && op.HasArgument("pad_l") && op.HasArgument("pad_b") &&
             op.HasArgument("pad_r")) {
    g.pads = {op.template GetSingleArgument<int>("pad_t", 0), op.template GetSingleArgument<int>("pad_l", 0),
              op.template GetSingleArgument<int>("pad_b", 0), op.template GetSingleArgument<int>("pad_r", 0)};
  }
  if (g.kernel.empty()) g.kernel.assign(2, 0);
  if (g.stride.empty()) g.stride.assign(g.kernel.size(), 1);
  if (g.pads.empty()) g.pads.assign(g.kernel.size() * 2, 0);
  if (g.dilation.empty()) g.dilation.assign(g.kernel.size(), 1);
  CAFFE_ENFORCE_EQ(g.stride.size(), g.kernel.size());
  CAFFE_ENFORCE_EQ(g.dilation.size(), g.kernel.size());
  CAFFE_ENFORCE_EQ(g.pads.size(), 2 * g.kernel.size());
  for (size_t d = 0; d < g.kernel.size(); ++d) {
    CAFFE_ENFORCE_GE(g.pads[d], 0);
    CAFFE_ENFORCE_GE(g.pads[g.kernel.size() + d], 0);
    CAFFE_ENFORCE(g.kernel[d],
                  "If you are doing convolution or pooling, you will need to set explicitly "
                  "the kernel size.");
    CAFFE_ENFORCE_GE(g.dilation[d], 0);
    CAFFE_ENFORCE_GE(g.stride[d], 0);
  }
  CAFFE_ENFORCE(g.order == "NCHW" || g.order == "NHWC", "Unknown storage order: ", g.order);
  return g;
}


// Parses and validates the convolution arguments exactly as the base class of
// the reference does; shared by Conv and ConvGradient (and, over a bare definition, by the net lowering).
ConvGeometry ParseConvGeometry(const OperatorBase& op);
ConvGeometry ParseConvGeometry(const OperatorDef& def);
bool IsSubnetGeometry(const ConvGeometry& g);   // 3x3 / s1 / p1 / d1 / g1 / NCHW
bool IsDefaultEngineGeometry(const ConvGeometry& g);   // any 2-D NCHW geometry (group >= 1)

// One 3x3 / stride 1 / pad 1 fp32 problem of the operator surface.  A Conv is a ConvGroup of one problem, a
// ConvGradient a ConvGradientGroup of one problem and one filter: all four operators run on a Conv3x3Runner.
struct Conv3x3Problem {
  const Tensor<HIPContext>* x = nullptr;
  const Tensor<HIPContext>* w = nullptr;
  const Tensor<HIPContext>* b = nullptr;     // forward: bias (or null); gradient: dY
  Tensor<HIPContext>* y = nullptr;           // forward: Y; gradient: dX (or null)
  int N = 0, C = 0, H = 0, W = 0, M = 0;
  Conv3x3Problem() {}
  Conv3x3Problem(const Tensor<HIPContext>& x_, const Tensor<HIPContext>& w_, const Tensor<HIPContext>* b_,
                 Tensor<HIPContext>* y_)
      : x(&x_), w(&w_), b(b_), y(y_), N(x_.dim32(0)), C(x_.dim32(1)), H(x_.dim32(2)), W(x_.dim32(3)), M(w_.dim32(0)) {}
};

// The launch path of the 3x3 engines: the packed filters (ops/filter_pack_cache.h), the split-operand engine's and the
// filter gradient's workspaces, the engine of each launch by the rule of ops/conv3x3_engine.h.  `what` is the text of
// a failed launch.
class Conv3x3Runner {
 public:
  // One launcher call per class of equal (M, C), classes in order of first appearance, per SSAD_MAX_CONV_PROBLEMS
  // problems; after one pack launch per layout for the filters written since.  dgrad = false: y = conv(x, w) + b under
  // `flags`.  dgrad = true: the data gradient, y (dX, C channels) from b (dY, M channels) on the flipped / transposed
  // pack, masked by x > 0 when flags has SSAD_CONV_MASK_AUX.
  void Forward(const vector<Conv3x3Problem>& probs, const string& algo, int flags, bool dgrad, const char* what,
               hipStream_t s);
  // dW (and db unless null) of one [M][C][3][3] filter, reduced over the problems `mine` that read it (SSAD_MAX_LEVELS
  // a launch, the later launches accumulating); overwrite, beta = 0 (conv_op_cudnn.cc:1037).
  void FilterGradient(const vector<Conv3x3Problem>& probs, const vector<int>& mine, float* dW, float* db, int M, int C,
                      const string& algo, const char* what, hipStream_t s);
  // want, flush, count, packed for one filter (the route of hip_algo = "grouped")
  const float* Pack(const Tensor<HIPContext>& filter, FilterPackCache::Kind kind, hipStream_t s);

 private:
  void FlushPacks(hipStream_t s);
  FilterPackCache cache_;
  SplitEngine split_;
  Tensor<HIPContext> wgrad_workspace_;     // grows to the largest launch seen
};

template <typename T, class Context>
class ConvOp final : public Operator<Context> {
 public:
  USE_OPERATOR_CONTEXT_FUNCTIONS;
  ConvOp(const OperatorDef& def, Workspace* ws)
      : Operator<Context>(def, ws),
        geom_(ParseConvGeometry(*this)),
        fuse_relu_(OperatorBase::GetSingleArgument<int>("fuse_relu", 0)),
        fuse_sigmoid_(OperatorBase::GetSingleArgument<int>("fuse_sigmoid", 0)),
        algo_(OperatorBase::GetSingleArgument<string>("hip_algo", "auto")) {
    if (!IsDefaultEngineGeometry(geom_))
      throw UnsupportedOperatorFeature("HIP Conv engines implement order=NCHW, 2-D only");
  }
  bool RunOnDevice() override;

 private:
  bool RunDefaultEngine();
  bool RunGrouped();
  bool RunFloat16();
  ConvGeometry geom_;
  int fuse_relu_;
  int fuse_sigmoid_;                    // Y = sigmoid(conv) (set by the net lowering: Conv -> Sigmoid; 3x3 fp32 path only)
  string algo_;
  Tensor<Context> packed_filter_;
  Conv3x3Runner runner_;
  Tensor<Context> col_buffer_;
  // float16 blobs: the filter and the bias as fp32, X and Y channel-blocked (Y as NCHW fp32 where M % 8)
  Tensor<Context> filter_f32_, bias_f32_, x_blocked_, out_blocked_;
  bool RunFloat16Pointwise();
};

template <typename T, class Context>
class ConvGradientOp final : public Operator<Context> {
 public:
  USE_OPERATOR_CONTEXT_FUNCTIONS;
  ConvGradientOp(const OperatorDef& def, Workspace* ws)
      : Operator<Context>(def, ws),
        geom_(ParseConvGeometry(*this)),
        no_bias_(OperatorBase::GetSingleArgument<int>("no_bias", 0)),
        relu_grad_on_input_(OperatorBase::GetSingleArgument<int>("relu_grad_on_input", 0)),
        algo_(OperatorBase::GetSingleArgument<string>("hip_algo", "auto")) {
    CAFFE_ENFORCE(!(no_bias_ && OutputSize() == 3),
                  "If bias is not present, you should not have 3 grad output.");
    if (!IsDefaultEngineGeometry(geom_))
      throw UnsupportedOperatorFeature(
          "HIP ConvGradient engines implement order=NCHW, 2-D only");
  }
  bool RunOnDevice() override;

 private:
  ConvGeometry geom_;
  bool no_bias_;
  int relu_grad_on_input_;
  string algo_;
  bool RunDefaultEngine();
  bool RunGrouped();
  bool RunFloat16();
  // the dX output, resized like X -- or null where the definition has none (conv_gradient_op.cc:35-77)
  Tensor<Context>* DataGradOutput();
  // dbias = the channel sums of dY [N][M][P] (nothing under no_bias)
  void EmitBiasGrad(const Tensor<Context>& dY, int N, int M, int P);
  // float16 blobs: dfilter and dbias from their fp32 sums
  void EmitFloat16FilterGrads(const Tensor<Context>& filter, int M);
  Tensor<Context> packed_filter_;
  Conv3x3Runner runner_;
  Tensor<Context> workspace_;
  Tensor<Context> col_buffer_;
  // float16 blobs: X and dY channel-blocked, the filter and bias gradients' fp32 sums, the filter as fp32, dX
  // channel-blocked (as NCHW fp32 where C % 8); the strided pointwise layer's subsampled X and upsampled dX
  Tensor<Context> x_blocked_, dy_blocked_, dfilter_f32_, dbias_f32_, filter_f32_, out_blocked_, x_subsampled_,
      dx_upsampled_;
  bool RunFloat16Pointwise();
};

}  // namespace caffe2
#endif
