// ConvGroup / ConvGradientGroup for HIPContext -- the operators the net lowering (ops/net_lowering.cc)
// emits for convolutions that are ready together: ConvShared's five FPN levels of one filter
// (detectron/lib/modeling/detector.py:449-482, retinanet_heads.py:97-152), the cls and bbox tower layer
// of equal depth.  The reference issues one cuDNN call per (level, layer) (conv_op_cudnn.cc:567-617,
// :1011-1058) and sums the five filter-gradient pieces of a shared filter with a separate Sum operator
// (caffe2/python/core.py:706-741); here a group is ONE multi-problem launch per (Cout, Cin) class -- the
// small levels fill the tail of the large ones -- and the filter-gradient launch reduces over every level
// of its filter, so the pieces and their Sum never exist.
//
//   ConvGroup          inputs  [X_0, W_0, (b_0), X_1, W_1, (b_1), ...]      outputs [Y_0, Y_1, ...]
//   ConvGradientGroup  inputs  [X_0, W_0, dY_0, X_1, W_1, dY_1, ...]
//                      outputs [dW_f ...] [db_f ...] [dX_i ...]   f = distinct filters, arg filter_index[i]
//
// Arguments are the member operators' own (conv_pool_op_base.h:45-194 geometry, fuse_relu,
// relu_grad_on_input, no_bias, hip_algo); the geometry must be 3x3 / stride 1 / pad 1 and the blobs fp32
// (the lowering only groups those).  Packs, engines and launches are the Conv3x3Runner's (ops/conv_op.h), as for a
// single Conv / ConvGradient; what is left here is argument parsing, checks and output shapes.
#include <atomic>

#include "ops/conv_op.h"
#include "ssad_kernels.h"

namespace caffe2 {

std::atomic<long long> g_filter_packs_issued{0};   // c2hip_counter("filter_packs")
std::atomic<long long> g_conv_launch_calls{0};     // c2hip_counter("conv_launch_calls")

namespace {

void CheckSubnetProblem(const Conv3x3Problem& p) {
  CAFFE_ENFORCE(p.x->IsType<float>() && p.w->IsType<float>(),
                "ConvGroup / ConvGradientGroup are fp32 operators (float16 blobs run as single Conv operators)");
  CAFFE_ENFORCE_EQ(p.x->ndim(), 4);
  CAFFE_ENFORCE_EQ(p.w->ndim(), 4);
  CAFFE_ENFORCE(p.w->dim32(1) == p.C, "Convolution op: input channels does not match: # of input channels ", p.C,
                " is not equal to kernel channels:", p.w->dim32(1));
  CAFFE_ENFORCE(p.w->dim32(2) == 3 && p.w->dim32(3) == 3);
}

}  // namespace

class ConvGroupOp final : public Operator<HIPContext> {
 public:
  ConvGroupOp(const OperatorDef& def, Workspace* ws)
      : Operator<HIPContext>(def, ws),
        geom_(ParseConvGeometry(*this)),
        fuse_relu_(GetSingleArgument<int>("fuse_relu", 0)),
        fuse_sigmoid_(GetSingleArgument<int>("fuse_sigmoid", 0)),
        algo_(GetSingleArgument<string>("hip_algo", "auto")) {
    CAFFE_ENFORCE(IsSubnetGeometry(geom_), "ConvGroup implements kernel 3 / stride 1 / pad 1 / group 1 / NCHW");
    CAFFE_ENFORCE(OutputSize() >= 1 && InputSize() % OutputSize() == 0, "ConvGroup: [X, W, (b)] per output");
    per_ = InputSize() / OutputSize();
    CAFFE_ENFORCE(per_ == 2 || per_ == 3, "ConvGroup: [X, W, (b)] per output");
  }

  bool RunOnDevice() override {
    const int k = OutputSize();
    vector<Conv3x3Problem> probs;
    for (int i = 0; i < k; ++i) {
      probs.emplace_back(Input(per_ * i), Input(per_ * i + 1), per_ == 3 ? &Input(per_ * i + 2) : nullptr, Output(i));
      const Conv3x3Problem& p = probs.back();
      CheckSubnetProblem(p);
      if (p.b) CAFFE_ENFORCE(p.b->ndim() == 1 && p.b->dim32(0) == p.M);
      p.y->Resize(p.N, p.M, p.H, p.W);
    }
    const int flags = (fuse_relu_ ? SSAD_CONV_RELU : 0) | (fuse_sigmoid_ ? SSAD_CONV_SIGMOID : 0);
    runner_.Forward(probs, algo_, flags, false, "ConvGroup launch failed", context_.hip_stream());
    return true;
  }

 private:
  ConvGeometry geom_;
  int fuse_relu_;
  int fuse_sigmoid_;
  string algo_;
  int per_ = 3;
  Conv3x3Runner runner_;
};

class ConvGradientGroupOp final : public Operator<HIPContext> {
 public:
  ConvGradientGroupOp(const OperatorDef& def, Workspace* ws)
      : Operator<HIPContext>(def, ws),
        geom_(ParseConvGeometry(*this)),
        no_bias_(GetSingleArgument<int>("no_bias", 0) != 0),
        relu_grad_on_input_(GetSingleArgument<int>("relu_grad_on_input", 0)),
        algo_(GetSingleArgument<string>("hip_algo", "auto")),
        filter_index_(GetRepeatedArgument<int>("filter_index")),
        n_filters_(GetSingleArgument<int>("n_filters", 0)) {
    CAFFE_ENFORCE(IsSubnetGeometry(geom_),
                  "ConvGradientGroup implements kernel 3 / stride 1 / pad 1 / group 1 / NCHW");
    CAFFE_ENFORCE(InputSize() % 3 == 0 && InputSize() >= 3, "ConvGradientGroup: [X, W, dY] per problem");
    k_ = InputSize() / 3;
    CAFFE_ENFORCE_EQ((int)filter_index_.size(), k_);
    CAFFE_ENFORCE(n_filters_ >= 1 && n_filters_ <= k_);
    const int fixed = n_filters_ * (no_bias_ ? 1 : 2);
    CAFFE_ENFORCE(OutputSize() == fixed || OutputSize() == fixed + k_,
                  "ConvGradientGroup: outputs are [dW_f ...] [db_f ...] and optionally one dX per problem");
    want_dx_ = OutputSize() == fixed + k_;
    for (int f : filter_index_) CAFFE_ENFORCE(f >= 0 && f < n_filters_);
  }

  bool RunOnDevice() override {
    vector<Conv3x3Problem> probs;
    const int fixed = n_filters_ * (no_bias_ ? 1 : 2);
    for (int i = 0; i < k_; ++i) {
      probs.emplace_back(Input(3 * i), Input(3 * i + 1), &Input(3 * i + 2), want_dx_ ? Output(fixed + i) : nullptr);
      const Conv3x3Problem& p = probs.back();
      CheckSubnetProblem(p);
      CAFFE_ENFORCE(p.b->ndim() == 4 && p.b->dim32(0) == p.N && p.b->dim32(1) == p.M && p.b->dim32(2) == p.H &&
                        p.b->dim32(3) == p.W,
                    "output gradient shape does not match the convolution output");
      if (p.y) p.y->ResizeLike(*p.x);
    }
    hipStream_t s = context_.hip_stream();

    // filter (+ bias) gradients: one launch per filter over all of its problems -- the reduction over
    // levels IS the autograd Sum of core.py:706-741
    for (int f = 0; f < n_filters_; ++f) {
      vector<int> mine;
      for (int i = 0; i < k_; ++i)
        if (filter_index_[i] == f) mine.push_back(i);
      CAFFE_ENFORCE(!mine.empty());
      const Conv3x3Problem& p0 = probs[mine[0]];
      for (int i : mine)
        CAFFE_ENFORCE(probs[i].w->raw_data() == p0.w->raw_data() && probs[i].M == p0.M && probs[i].C == p0.C,
                      "problems of one filter_index must read one filter blob");
      auto* dW = Output(f);
      dW->ResizeLike(*p0.w);
      float* db = nullptr;
      if (!no_bias_) {
        auto* dbt = Output(n_filters_ + f);
        dbt->Resize(p0.M);
        db = dbt->mutable_data<float>();
      }
      runner_.FilterGradient(probs, mine, dW->mutable_data<float>(), db, p0.M, p0.C, algo_,
                             "ConvGradientGroup (filter) launch failed", s);
    }
    // data gradients: the forward kernel on the flipped / transposed pack, dX has C channels
    if (want_dx_)
      runner_.Forward(probs, algo_, relu_grad_on_input_ ? SSAD_CONV_MASK_AUX : 0, true,
                      "ConvGradientGroup (data) launch failed", s);
    return true;
  }

 private:
  ConvGeometry geom_;
  bool no_bias_;
  int relu_grad_on_input_;
  string algo_;
  vector<int> filter_index_;
  int n_filters_;
  int k_ = 0;
  bool want_dx_ = false;
  Conv3x3Runner runner_;
};

REGISTER_HIP_OPERATOR(ConvGroup, ConvGroupOp);
REGISTER_HIP_OPERATOR(ConvGradientGroup, ConvGradientGroupOp);

OPERATOR_SCHEMA(ConvGroup)
    .NumInputs(2, INT_MAX)
    .NumOutputs(1, INT_MAX)
    .SetDoc("Convolutions of equal arguments that are ready together, one multi-problem launch per "
            "(Cout, Cin) class; emitted by the net lowering, [X, W, (b)] per output.");
OPERATOR_SCHEMA(ConvGradientGroup)
    .NumInputs(3, INT_MAX)
    .NumOutputs(1, INT_MAX)
    .Arg("filter_index", "per problem: which of the n_filters distinct filters it reads")
    .Arg("n_filters", "number of distinct filters = number of dW (and db) outputs")
    .SetDoc("ConvGradients that are ready together; the filter gradient of a filter is reduced over all of "
            "its problems in one launch (the Sum of core.py:706-741 absorbed).");
NO_GRADIENT(ConvGroup);
NO_GRADIENT(ConvGradientGroup);

}  // namespace caffe2
