// GroupSpatialSoftmax(+Gradient) and SoftmaxFocalLoss(+Gradient) for HIPContext -- the
// RETINANET.SOFTMAX classification head, built by detectron/lib/modeling/retinanet_heads.py:
// 154-159 (test-mode probabilities) and :292-304 (the training loss).
//
// Contracts (arguments, defaults, inputs/outputs, gradient makers) follow
// caffe2/modules/detectron/group_spatial_softmax_op.{h,cc} and softmax_focal_loss_op.{h,cc};
// like the reference there is no CPU implementation (the CPU registrations raise
// "Not Implemented").  The kernels are csrc/kernels/softmax_focal.hip.
#include "c2/operator.h"
#include "ssad_kernels.h"

namespace caffe2 {

namespace {
void Launched(int rc, const char* what) { CAFFE_ENFORCE_EQ(rc, 0, what, " launch failed"); }

void CheckOrder(OperatorBase* op) {
  CAFFE_ENFORCE_EQ(op->GetSingleArgument<string>("order", "NCHW"), "NCHW",
                   "Only NCHW order is supported right now.");
}

// N, D, H, W of a 4-D tensor whose channels are num_anchors groups of num_classes
template <class Ctx>
void GroupDims(const Tensor<Ctx>& X, int num_classes, int* N, int* D, int* H, int* W) {
  CAFFE_ENFORCE_EQ(X.ndim(), 4, "scores must be N x (A*num_classes) x H x W");
  CAFFE_ENFORCE_GT(num_classes, 0);
  *N = X.dim32(0); *D = X.dim32(1); *H = X.dim32(2); *W = X.dim32(3);
  CAFFE_ENFORCE_EQ(*D % num_classes, 0, "channel dim must be num_anchors * num_classes");
}
}  // namespace

// ---------------------------------------------------------------------------
// GroupSpatialSoftmax
// ---------------------------------------------------------------------------
template <typename T, class Context>
class GroupSpatialSoftmaxOp final : public Operator<Context> {
 public:
  GroupSpatialSoftmaxOp(const OperatorDef& def, Workspace* ws)
      : Operator<Context>(def, ws),
        num_classes_(OperatorBase::GetSingleArgument<int>("num_classes", 81)) {
    CheckOrder(this);
  }
  USE_OPERATOR_CONTEXT_FUNCTIONS;
  bool RunOnDevice() override { CAFFE_NOT_IMPLEMENTED; }   // no CPU implementation

 protected:
  int num_classes_;
};

template <typename T, class Context>
class GroupSpatialSoftmaxGradientOp final : public Operator<Context> {
 public:
  GroupSpatialSoftmaxGradientOp(const OperatorDef& def, Workspace* ws)
      : Operator<Context>(def, ws),
        num_classes_(OperatorBase::GetSingleArgument<int>("num_classes", 81)) {
    CheckOrder(this);
  }
  USE_OPERATOR_CONTEXT_FUNCTIONS;
  bool RunOnDevice() override { CAFFE_NOT_IMPLEMENTED; }

 protected:
  int num_classes_;
};

template <>
bool GroupSpatialSoftmaxOp<float, HIPContext>::RunOnDevice() {
  auto& X = Input(0);    // logits
  auto* P = Output(0);   // probabilities
  int N, D, H, W;
  GroupDims(X, num_classes_, &N, &D, &H, &W);
  P->ResizeLike(X);
  if (X.size() == 0) return true;
  Launched(ssad_group_spatial_softmax(X.data<float>(), P->mutable_data<float>(), N, D / num_classes_,
                                      num_classes_, H, W, 0, context_.hip_stream()),
           "GroupSpatialSoftmax");
  return true;
}

template <>
bool GroupSpatialSoftmaxGradientOp<float, HIPContext>::RunOnDevice() {
  auto& Y = Input(0);    // probabilities
  auto& dY = Input(1);
  auto* dX = Output(0);
  int N, D, H, W;
  GroupDims(Y, num_classes_, &N, &D, &H, &W);
  CAFFE_ENFORCE_EQ(dY.size(), Y.size(), "d_probabilities must have the probabilities' shape");
  dX->ResizeLike(Y);
  if (Y.size() == 0) return true;
  Launched(ssad_group_spatial_softmax_grad(Y.data<float>(), dY.data<float>(), dX->mutable_data<float>(), N,
                                           D / num_classes_, num_classes_, H, W, context_.hip_stream()),
           "GroupSpatialSoftmaxGradient");
  return true;
}

// ---------------------------------------------------------------------------
// SoftmaxFocalLoss
// ---------------------------------------------------------------------------
template <typename T, class Context>
class SoftmaxFocalLossOp final : public Operator<Context> {
 public:
  SoftmaxFocalLossOp(const OperatorDef& def, Workspace* ws)
      : Operator<Context>(def, ws),
        scale_(OperatorBase::GetSingleArgument<float>("scale", 1.f)),
        gamma_(OperatorBase::GetSingleArgument<float>("gamma", 1.f)),
        alpha_(OperatorBase::GetSingleArgument<float>("alpha", 0.25f)),
        num_classes_(OperatorBase::GetSingleArgument<int>("num_classes", 81)) {
    CAFFE_ENFORCE(scale_ >= 0);
    CheckOrder(this);
  }
  USE_OPERATOR_CONTEXT_FUNCTIONS;
  bool RunOnDevice() override { CAFFE_NOT_IMPLEMENTED; }

 protected:
  float scale_;
  float gamma_;
  float alpha_;
  int num_classes_;
  Tensor<Context> partials_;   // reduction scratch (the reference keeps a full-size losses_ here)
};

template <typename T, class Context>
class SoftmaxFocalLossGradientOp final : public Operator<Context> {
 public:
  SoftmaxFocalLossGradientOp(const OperatorDef& def, Workspace* ws)
      : Operator<Context>(def, ws),
        scale_(OperatorBase::GetSingleArgument<float>("scale", 1.f)),
        gamma_(OperatorBase::GetSingleArgument<float>("gamma", 1.f)),
        alpha_(OperatorBase::GetSingleArgument<float>("alpha", 0.25f)),
        num_classes_(OperatorBase::GetSingleArgument<int>("num_classes", 81)) {
    CAFFE_ENFORCE(scale_ >= 0);
    CheckOrder(this);
  }
  USE_OPERATOR_CONTEXT_FUNCTIONS;
  bool RunOnDevice() override { CAFFE_NOT_IMPLEMENTED; }

 protected:
  float scale_;
  float gamma_;
  float alpha_;
  int num_classes_;
};

namespace {
template <class Ctx>
ssad_softmax_focal_level SoftmaxLevel(const Tensor<Ctx>& X, const Tensor<Ctx>& T, const Tensor<Ctx>& wp,
                                      int num_classes) {
  int N, D, H, W;
  GroupDims(X, num_classes, &N, &D, &H, &W);
  CAFFE_ENFORCE_EQ(T.size(), (TIndex)N * (D / num_classes) * H * W, "labels must be N x num_anchors x H x W");
  CAFFE_ENFORCE_GE(wp.size(), 1);
  return ssad_softmax_focal_level{X.template data<float>(), T.template data<int>(), nullptr, nullptr, N, D, H, W};
}
}  // namespace

template <>
bool SoftmaxFocalLossOp<float, HIPContext>::RunOnDevice() {
  auto& X = Input(0);           // logits
  auto& T = Input(1);           // labels
  auto& wp = Input(2);          // number of foreground anchors
  auto* avg_loss = Output(0);
  auto* P = Output(1);          // softmax probabilities, re-used by the gradient
  ssad_softmax_focal_level lv = SoftmaxLevel(X, T, wp, num_classes_);
  avg_loss->Resize(vector<TIndex>());
  P->ResizeLike(X);             // 4-D as the schema documents it (the reference flattens it)
  lv.out = avg_loss->mutable_data<float>();
  lv.prob = P->mutable_data<float>();
  hipStream_t s = context_.hip_stream();
  if (X.size() == 0) {
    Launched(ssad_fill(lv.out, 0.0f, 1, s), "SoftmaxFocalLoss");
    return true;
  }
  const size_t wsb = ssad_softmax_focal_loss_workspace_bytes(1);
  partials_.Resize((TIndex)wsb);
  const ssad_focal_params Pm{gamma_, alpha_, num_classes_, scale_};
  Launched(ssad_softmax_focal_loss_forward(&lv, 1, wp.data<float>(), &Pm, partials_.mutable_data<uint8_t>(), wsb, s),
           "SoftmaxFocalLoss");
  return true;
}

template <>
bool SoftmaxFocalLossGradientOp<float, HIPContext>::RunOnDevice() {
  auto& X = Input(0);
  auto& T = Input(1);
  auto& wp = Input(2);
  auto& P = Input(3);           // output 1 of the forward
  auto& d_avg_loss = Input(4);
  auto* dX = Output(0);
  ssad_softmax_focal_level lv = SoftmaxLevel(X, T, wp, num_classes_);
  CAFFE_ENFORCE_EQ(P.size(), X.size(), "probabilities must have the logits' size");
  CAFFE_ENFORCE_GE(d_avg_loss.size(), 1);
  dX->ResizeLike(X);
  if (X.size() == 0) return true;
  lv.prob = const_cast<float*>(P.data<float>());
  lv.out = dX->mutable_data<float>();
  const ssad_focal_params Pm{gamma_, alpha_, num_classes_, scale_};
  Launched(ssad_softmax_focal_loss_backward(&lv, 1, wp.data<float>(), d_avg_loss.data<float>(), 0, &Pm,
                                            context_.hip_stream()),
           "SoftmaxFocalLossGradient");
  return true;
}

REGISTER_CPU_OPERATOR(GroupSpatialSoftmax, GroupSpatialSoftmaxOp<float, CPUContext>);
REGISTER_CPU_OPERATOR(GroupSpatialSoftmaxGradient, GroupSpatialSoftmaxGradientOp<float, CPUContext>);
REGISTER_CPU_OPERATOR(SoftmaxFocalLoss, SoftmaxFocalLossOp<float, CPUContext>);
REGISTER_CPU_OPERATOR(SoftmaxFocalLossGradient, SoftmaxFocalLossGradientOp<float, CPUContext>);
REGISTER_HIP_OPERATOR(GroupSpatialSoftmax, GroupSpatialSoftmaxOp<float, HIPContext>);
REGISTER_HIP_OPERATOR(GroupSpatialSoftmaxGradient, GroupSpatialSoftmaxGradientOp<float, HIPContext>);
REGISTER_HIP_OPERATOR(SoftmaxFocalLoss, SoftmaxFocalLossOp<float, HIPContext>);
REGISTER_HIP_OPERATOR(SoftmaxFocalLossGradient, SoftmaxFocalLossGradientOp<float, HIPContext>);

OPERATOR_SCHEMA(GroupSpatialSoftmax)
    .NumInputs(1)
    .NumOutputs(1)
    .Arg("num_classes", "(int) default 81; number of classes in each softmax group.")
    .Input(0, "scores", "4D tensor (N, A * num_classes, H, W): A groups of num_classes softmax inputs.")
    .Output(0, "probabilities", "4D tensor of the same shape; each group's num_classes values sum to 1.");
OPERATOR_SCHEMA(GroupSpatialSoftmaxGradient).NumInputs(2).NumOutputs(1);
OPERATOR_SCHEMA(SoftmaxFocalLoss)
    .NumInputs(3)
    .NumOutputs(2)
    .Arg("scale", "(float) default 1.0; multiply the loss by this scale factor.")
    .Arg("alpha", "(float) default 0.25; Focal Loss's alpha hyper-parameter.")
    .Arg("gamma", "(float) default 1.0; Focal Loss's gamma hyper-parameter.")
    .Arg("num_classes", "(int) default 81; number of classes in each softmax group.")
    .Input(0, "scores", "4D tensor (N, A * num_classes, H, W).")
    .Input(1, "labels", "4D int32 tensor (N, A, H, W): -1 ignore, else a class in [0, num_classes - 1].")
    .Input(2, "normalizer", "Scalar; the loss is normalized by 1 / max(1, normalizer).")
    .Output(0, "loss", "Scalar loss.")
    .Output(1, "probabilities", "4D tensor of softmax probabilities (N, A * num_classes, H, W).");
OPERATOR_SCHEMA(SoftmaxFocalLossGradient).NumInputs(5).NumOutputs(1);

class GetGroupSpatialSoftmaxGradient : public GradientMakerBase {
  using GradientMakerBase::GradientMakerBase;
  vector<OperatorDef> GetGradientDefs() override {
    return SingleGradientDef("GroupSpatialSoftmaxGradient", "", vector<string>{O(0), GO(0)},
                             vector<string>{GI(0)});
  }
};
REGISTER_GRADIENT(GroupSpatialSoftmax, GetGroupSpatialSoftmaxGradient);

class GetSoftmaxFocalLossGradient : public GradientMakerBase {
  using GradientMakerBase::GradientMakerBase;
  vector<OperatorDef> GetGradientDefs() override {
    return SingleGradientDef("SoftmaxFocalLossGradient", "",
                             vector<string>{I(0), I(1), I(2), O(1), GO(0)}, vector<string>{GI(0)});
  }
};
REGISTER_GRADIENT(SoftmaxFocalLoss, GetSoftmaxFocalLossGradient);

}  // namespace caffe2
