// yolo_box.hpp — TBox's overlap / box_iou (ntypes.pas:1059-1108) in the
// single-precision form the reference computes, shared by yolo_loss.hip and
// detections.hip.  Compiled with -ffp-contract=off; [s] marks a single.
#pragma once
#include <hip/hip_runtime.h>

namespace tns {
namespace {

struct Box {
  float x, y, w, h;
};

// overlap (ntypes.pas:1059-1075), singles throughout
__device__ __forceinline__ float overlap(float x1, float w1, float x2, float w2) {
  const float l1 = x1 - w1 / 2.0f;  // [s] w1/2 [s], then the difference [s]
  const float l2 = x2 - w2 / 2.0f;  // [s]
  const float left = l1 > l2 ? l1 : l2;
  const float r1 = x1 + w1 / 2.0f;  // [s]
  const float r2 = x2 + w2 / 2.0f;  // [s]
  const float right = r1 < r2 ? r1 : r2;
  return right - left;  // [s]
}

// box_iou (ntypes.pas:1077-1108): I = box_intersection, U = a.w*a.h + b.w*b.h
// - I; 0 when either is 0
__device__ __forceinline__ float box_iou(const Box& a, const Box& b) {
  const float w = overlap(a.x, a.w, b.x, b.w);
  const float h = overlap(a.y, a.h, b.y, b.h);
  const float I = (w < 0.0f || h < 0.0f) ? 0.0f : w * h;  // [s]
  const float U = a.w * a.h + b.w * b.h - I;  // [s] two products, their sum, minus I
  if (I == 0.0f || U == 0.0f) return 0.0f;
  return I / U;  // [s]
}

}  // namespace
}  // namespace tns
