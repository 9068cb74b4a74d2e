// yolo_box.hpp — TBox's overlap / box_iou (ntypes.pas:1059-1108) in the
// single-precision form the reference computes, and the box correction the
// detections end with, shared by yolo_loss.hip, detections.hip and
// region.hip.  Compiled with -ffp-contract=off; [s] marks a single.
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

// TYoloLayer.correctBoxes (nyololayer.pas:452-498) and correct_yolo_boxes
// (nregionlayer.pas:607-653), the same expressions, on one box; imW, imH are
// the image's extents.  [d] double, [i] integer.
__device__ __forceinline__ Box correct_box(Box b, int netW, int netH, int imW, int imH,
                                           int relative, int letter) {
  long long new_w = netW, new_h = netH;  // [i]
  if (letter) {
    // (netw / w) [d] < (neth / h) [d]: integer / integer is a real
    if ((double)netW / (double)imW < (double)netH / (double)imH)
      new_h = ((long long)imH * netW) / imW;  // [i] (h * netw) div w
    else
      new_w = ((long long)imW * netH) / imH;  // [i] (w * neth) div h
  }
  const float deltaw = (float)(netW - new_w);  // [i] difference, assigned to a single
  const float deltah = (float)(netH - new_h);
  const float ratiow = (float)((double)new_w / (double)netW);  // [d] quotient, rounded once
  const float ratioh = (float)((double)new_h / (double)netH);
  // (b.x - deltaw / 2.0 / netw) / ratiow: deltaw / 2.0 [s], / netw [s], the
  // difference [s], / ratiow [s]
  b.x = (b.x - deltaw / 2.0f / (float)netW) / ratiow;
  b.y = (b.y - deltah / 2.0f / (float)netH) / ratioh;
  b.w = b.w * (1.0f / ratiow);  // (1 / ratiow) [s], the product [s]
  b.h = b.h * (1.0f / ratioh);
  if (!relative) {
    b.x = b.x * (float)imW;  // [s] single * integer
    b.w = b.w * (float)imW;
    b.y = b.y * (float)imH;
    b.h = b.h * (float)imH;
  }
  return b;
}

}  // namespace
}  // namespace tns
