/*
 * tns.h — C ABI of libtensorium_hip.so, the MI355X (gfx950) backend for
 * Tensorium's fp32 SGEMM + im2col-convolution hot path.
 *
 * Two boundaries, both plain cdecl (SysV x86-64), no C++ or torch types:
 *
 *  A. Op-table drop-ins (host pointers).  Each function has exactly the
 *     parameter list of one TTensor<Single> class-var procedure pointer
 *     (source/ntensors.pas:345-385, bound in TTensorOps.initSingle,
 *     ntensors.pas:12651-12758).  A Pascal maintainer assigns e.g.
 *       TSingleTensor.gemm := @tns_cblas_sgemm;
 *     after initSingle, exactly like the USE_OPENBLAS / USE_MKL overrides at
 *     ntensors.pas:12735-12756.  These return void (the Pascal pointer types
 *     have no status channel): a failure is recorded in a thread-local error
 *     string read with tns_last_error(); an optional fatal hook
 *     (tns_set_error_hook) lets the binding raise like SAFE_CALL does
 *     (nncuda.pas:216-275).  The shim stages host buffers through device
 *     scratch that it owns; results are complete when the call returns.
 *
 *  B. Device-resident backend (device pointers + element offsets), the HIP
 *     twin of TNNCuda<T> (source/nncuda.pas:35-157) / TNNOpenCL<T>
 *     (source/nnopencl.pas:222-319).  Calls are stream-ordered and
 *     asynchronous on the context's stream; tns_hip_finish() synchronises,
 *     as TNNCuda.finish does (nncuda.pas:1575).  Every call returns a status
 *     (0 = TNS_OK); tns_last_error() carries the message.
 *
 * Enumerations keep the reference's ordinal values: CBLAS_LAYOUT /
 * CBLAS_TRANSPOSE (ntensors.pas:106-128, {$Z4} => 4-byte enums) and
 * TActivationType (ntypes.pas:66-71).
 */
#ifndef TNS_H
#define TNS_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TNS_ABI_VERSION 1

/* ---- enums (reference ordinals) ---------------------------------------- */
enum { TNS_CblasRowMajor = 101, TNS_CblasColMajor = 102 };           /* ntensors.pas:106-107 */
enum { TNS_CblasNoTrans = 111, TNS_CblasTrans = 112 };               /* ntensors.pas:119-120 */

/* TActivationType, ntypes.pas:66-71 */
enum {
  TNS_acLOGISTIC = 0, TNS_acRELU = 1, TNS_acRELU6 = 2, TNS_acRELIE = 3,
  TNS_acLINEAR = 4, TNS_acRAMP = 5, TNS_acTANH = 6, TNS_acPLSE = 7,
  TNS_acREVLEAKY = 8, TNS_acLEAKY = 9, TNS_acELU = 10, TNS_acLOGGY = 11,
  TNS_acSTAIR = 12, TNS_acHARDTAN = 13, TNS_acLHTAN = 14, TNS_acSELU = 15
};

/* status codes (boundary B) */
enum {
  TNS_OK = 0,
  TNS_ERR_ARG = 1,        /* invalid argument (shape, enum, null pointer) */
  TNS_ERR_HIP = 2,        /* a HIP runtime call failed                    */
  TNS_ERR_NOMEM = 3,      /* device allocation failed                     */
  TNS_ERR_UNSUPPORTED = 4 /* enum value the backend does not implement    */
};

/* ---- library / error channel ------------------------------------------- */
int         tns_abi_version(void);
const char* tns_last_error(void);          /* thread-local, "" when none   */
void        tns_clear_error(void);
typedef void (*tns_error_hook_t)(int code, const char* msg);
void        tns_set_error_hook(tns_error_hook_t hook);
int         tns_device_count(void);

/* =========================================================================
 * A. Op-table drop-ins (host pointers)
 * ========================================================================= */

/* TTensor<Single>.gemm  — ntensors.pas:345-347, CPU impl cblas_sgemm
 * ntensors.pas:2231-2286.  Row-major only (Order is accepted and ignored,
 * as the reference ignores it).  beta<>1 pre-scales C (beta=0 => 0*C, so
 * NaN/Inf in C propagate, ntensors.pas:2259-2261). */
void tns_cblas_sgemm(int32_t Order, int32_t TransA, int32_t TransB,
                     int64_t M, int64_t N, int64_t K, float ALPHA,
                     const float* A, int64_t lda, const float* B, int64_t ldb,
                     float BETA, float* C, int64_t ldc);

/* TTensor<Single>.gemmStridedBatched — ntensors.pas:348-351, CPU impl
 * cblas_sgemm_batch_strided ntensors.pas:2288-2304. */
void tns_cblas_sgemm_batch_strided(int32_t Layout, int32_t TransA, int32_t TransB,
                                   int64_t M, int64_t N, int64_t K, float alpha,
                                   const float* A, int64_t lda, int64_t strideA,
                                   const float* B, int64_t ldb, int64_t strideB,
                                   float beta, float* C, int64_t ldc, int64_t strideC,
                                   int64_t batch_size);

/* TTensor<Single>.im2Colvv — ntensors.pas:362-366, CPU impl sim2Col
 * ntensors.pas:11415-11491.  multiThread is a Pascal boolean (1 byte). */
void tns_im2col(int64_t aChannels, int64_t aHeight, int64_t aWidth,
                int64_t kernelHeight, int64_t kernelWidth, int64_t padHeight,
                int64_t padWidth, int64_t strideY, int64_t strideX,
                int64_t dilationY, int64_t dilationX,
                const float* inData, int64_t inOffset,
                float* outData, int64_t outOffset, uint8_t multiThread);

/* TTensor<Single>.col2imvv — ntensors.pas:367-371, CPU impl scol2im
 * ntensors.pas:11717-11763 (accumulates into im; never zeroes it). */
void tns_col2im(int64_t aChannels, int64_t aHeight, int64_t aWidth,
                int64_t kernelHeight, int64_t kernelWidth, int64_t padHeight,
                int64_t padWidth, int64_t strideY, int64_t strideX,
                int64_t dilationY, int64_t dilationX,
                const float* inData, int64_t inOffset,
                float* outData, int64_t outOffset, int64_t batch,
                uint8_t multiThread);

/* TTensor<Single>.im2colStridedBatchedvv — ntensors.pas:372-378, CPU impl
 * sim2colStridedBatched ntensors.pas:11493-11532. */
void tns_im2col_strided_batched(int64_t aChannels, int64_t aHeight, int64_t aWidth,
                                int64_t kernelHeight, int64_t kernelWidth,
                                int64_t padHeight, int64_t padWidth,
                                int64_t strideY, int64_t strideX,
                                int64_t dilationY, int64_t dilationX,
                                const float* im, int64_t imStride, int64_t imOffset,
                                float* col, int64_t colStride, int64_t colOffset,
                                int64_t batchCount);

/* TTensor<Single>.col2imStridedBatchedvv — ntensors.pas:379-385, CPU impl
 * scol2imStridedBatched ntensors.pas:11833-11879. */
void tns_col2im_strided_batched(int64_t aChannels, int64_t aHeight, int64_t aWidth,
                                int64_t kernelHeight, int64_t kernelWidth,
                                int64_t padHeight, int64_t padWidth,
                                int64_t strideY, int64_t strideX,
                                int64_t dilationY, int64_t dilationX,
                                const float* inData, int64_t inStride, int64_t inOffset,
                                float* outData, int64_t outStride, int64_t outOffset,
                                int64_t batchCount);

/* =========================================================================
 * B. Device-resident backend (TNNCuda<T> twin).  Pointers are device
 *    pointers (hipMalloc / torch); offsets are in ELEMENTS, as TCUMem+offset.
 * ========================================================================= */
typedef struct tns_ctx tns_ctx;

/* TNNCuda.Create(deviceIndex) — nncuda.pas:448-467.  Creates its own
 * non-blocking stream unless one is attached with tns_hip_set_stream. */
int  tns_hip_create(int32_t deviceIndex, tns_ctx** out);
int  tns_hip_destroy(tns_ctx* ctx);
int  tns_hip_set_stream(tns_ctx* ctx, void* hipStream);   /* hipStream_t */
/* The context's stream, after it has been made to wait for any pipelined
 * conv-backward dW products still pending on the side stream
 * (TNS_OPT_BWD_OVERLAP = 2), so work enqueued on it sees their results. */
void* tns_hip_get_stream(tns_ctx* ctx);   /* NULL on error: tns_last_error() */
/* Pipelined conv backward (TNS_OPT_BWD_OVERLAP = 2): the number of dW
 * products still pending on the side stream (0 once joined; -1 for a null
 * context).  Diagnostic: it shows which calls left the pipeline running. */
int  tns_hip_pending_dw(tns_ctx* ctx);
int  tns_hip_finish(tns_ctx* ctx);                         /* nncuda.pas:1575 */

/* createDeviceBuffer / freeDeviceBuffer / writeBuffer / readBuffer —
 * nncuda.pas:104-107 (sizes in BYTES for copies, as the reference). */
int  tns_hip_malloc(tns_ctx* ctx, int64_t nElements, float** out);
int  tns_hip_free(tns_ctx* ctx, float* p);
int  tns_hip_write_buffer(tns_ctx* ctx, float* dev, int64_t bytes, const void* host);
int  tns_hip_read_buffer(tns_ctx* ctx, const float* dev, int64_t bytes, void* host);

/* TNNCuda.gemm — nncuda.pas:624-725.  Same semantics as cblas_sgemm. */
int tns_hip_gemm(tns_ctx* ctx, uint8_t transA, uint8_t transB,
                 int64_t M, int64_t N, int64_t K, float ALPHA,
                 const float* A, int64_t aOffset, int64_t lda,
                 const float* B, int64_t bOffset, int64_t ldb,
                 float BETA, float* C, int64_t cOffset, int64_t ldc);

/* TNNCuda.gemmStridedBatched — nncuda.pas:809.  strideA = 0 shares A
 * (conv weights, nConvolutionLayer.pas:1078). */
int tns_hip_gemm_strided_batched(tns_ctx* ctx, uint8_t transA, uint8_t transB,
                                 int64_t M, int64_t N, int64_t K, float ALPHA,
                                 const float* A, int64_t aOffset, int64_t lda, int64_t strideA,
                                 const float* B, int64_t bOffset, int64_t ldb, int64_t strideB,
                                 float BETA, float* C, int64_t cOffset, int64_t ldc, int64_t strideC,
                                 int64_t batchCount);

/* TNNCuda.gemmBatched — nncuda.pas:727-760 (cublasSgemmBatched_64 over
 * arrays of matrix pointers).  A, B, C are arrays of batchCount pointers,
 * device-resident as the reference builds them with writeBuffer
 * (nConvolutionLayer.pas:1083-1085) or host-resident; the element offsets
 * apply to every entry.  The arrays are read in stream order (the call
 * waits for them); equally spaced entries whose GEMMs are independent (no
 * C entry overlaps another C entry or any A / B entry) run as one
 * strided-batched launch, all others GEMM by GEMM in array order, so an
 * entry may read what an earlier one wrote.  Results as tns_hip_gemm. */
int tns_hip_gemm_batched(tns_ctx* ctx, uint8_t transA, uint8_t transB,
                         int64_t M, int64_t N, int64_t K, float ALPHA,
                         const float* const* A, int64_t aOffset, int64_t lda,
                         const float* const* B, int64_t bOffset, int64_t ldb,
                         float BETA, float* const* C, int64_t cOffset, int64_t ldc,
                         int64_t batchCount);

/* TNNCuda.im2col — nncuda.pas:1144 (output layout = CPU sim2Col). */
int tns_hip_im2col(tns_ctx* ctx, int64_t aChannels, int64_t aHeight, int64_t aWidth,
                   int64_t kernelHeight, int64_t kernelWidth, int64_t padHeight, int64_t padWidth,
                   int64_t strideY, int64_t strideX, int64_t dilationY, int64_t dilationX,
                   const float* im, int64_t imOffset, float* col, int64_t colOffset);

/* Strided-batched im2col (one launch for the whole batch). */
int tns_hip_im2col_strided_batched(tns_ctx* ctx, int64_t aChannels, int64_t aHeight, int64_t aWidth,
                   int64_t kernelHeight, int64_t kernelWidth, int64_t padHeight, int64_t padWidth,
                   int64_t strideY, int64_t strideX, int64_t dilationY, int64_t dilationX,
                   const float* im, int64_t imStride, int64_t imOffset,
                   float* col, int64_t colStride, int64_t colOffset, int64_t batchCount);

/* TNNCuda.col2im — nncuda.pas:1212.  Race-free gather; per-pixel sum in the
 * CPU scol2im's ascending kernel-index order (ntensors.pas:11650-11715),
 * including its dilation formula (input_row := (kernel_row-pad)*dil). */
int tns_hip_col2im(tns_ctx* ctx, int64_t aChannels, int64_t aHeight, int64_t aWidth,
                   int64_t kernelHeight, int64_t kernelWidth, int64_t padHeight, int64_t padWidth,
                   int64_t strideY, int64_t strideX, int64_t dilationY, int64_t dilationX,
                   const float* col, int64_t colOffset, float* im, int64_t imOffset);

int tns_hip_col2im_strided_batched(tns_ctx* ctx, int64_t aChannels, int64_t aHeight, int64_t aWidth,
                   int64_t kernelHeight, int64_t kernelWidth, int64_t padHeight, int64_t padWidth,
                   int64_t strideY, int64_t strideX, int64_t dilationY, int64_t dilationX,
                   const float* col, int64_t colStride, int64_t colOffset,
                   float* im, int64_t imStride, int64_t imOffset, int64_t batchCount);

/* TNNCuda.forwardBias — nncuda.pas:582.  dst[(b*srcSize+i)*bs + j] += src[i*incb],
 * bs = dstSize/(srcSize*batch)  (vsAddB, ntensors.pas:4066-4093). */
int tns_hip_forward_bias(tns_ctx* ctx, int64_t dstSize, float* dst, int64_t offset,
                         int64_t srcSize, const float* src, int64_t incb, int64_t batch);

/* TNNCuda.backwardBias — dst[i*incb] += sum_b sum_j src[(b*dstSize+i)*bs + j]
 * (addSums, ntensors.pas:7729-7781).  incb >= 1 here and in forwardBias /
 * forwardScale / forwardScaleAdd (TNS_ERR_ARG otherwise). */
int tns_hip_backward_bias(tns_ctx* ctx, int64_t dstSize, float* dst, int64_t srcSize,
                          const float* src, int64_t srcOffset, int64_t incb, int64_t batch);

/* TNNCuda.ActivateArray / DeriveArray — nncuda.pas:524, 562; formulas
 * nactivation.pas:272-501, 508-717. */
int tns_hip_activate_array(tns_ctx* ctx, int64_t N, float* x, int64_t offset, int32_t activation);
int tns_hip_derive_array(tns_ctx* ctx, int64_t N, const float* x, int64_t offset,
                         int32_t activation, float* delta);

/* BLAS-1 / elementwise support (TNNCuda.axpy/scale/fill/copy/clamp).
 * TNS_ERR_ARG for N < 0, a null operand with N > 0, an increment < 1 on an
 * operand that is written, or < 0 on one that is only read (0 broadcasts). */
int tns_hip_axpy(tns_ctx* ctx, int64_t N, float a, const float* x, int64_t xOffset, int64_t incx,
                 float* y, int64_t yOffset, int64_t incy);
int tns_hip_scale(tns_ctx* ctx, int64_t N, float a, float* x, int64_t stride);
/* TConnectedLayer.update (nconnectedlayer.pas:324-359) /
 * TConvolutionalLayer.update (nConvolutionLayer.pas:673-705) in one pass:
 * biases += lrOverBatch*bias_updates, bias_updates *= momentum, the same for
 * scales (NULL pair when the layer has no batch norm), weight_updates +=
 * negDecayTimesBatch*weights, weights += lrOverBatch*weight_updates,
 * weight_updates *= momentum (each axpy one FMA, each scale one multiply).
 * The caller computes lrOverBatch = learning_rate / batch and
 * negDecayTimesBatch = -decay * batch in single precision as the reference. */
int tns_hip_sgd_update(tns_ctx* ctx, int64_t nWeights, float* weights, float* weight_updates,
                       int64_t n, float* biases, float* bias_updates, float* scales,
                       float* scale_updates, float lrOverBatch, float negDecayTimesBatch,
                       float momentum);
int tns_hip_fill(tns_ctx* ctx, int64_t N, float* x, int64_t offset, float val, int64_t stride);
int tns_hip_copy(tns_ctx* ctx, int64_t N, const float* src, int64_t srcOffset, int64_t inca,
                 float* dst, int64_t dstOffset, int64_t incb);
int tns_hip_clamp(tns_ctx* ctx, int64_t N, float alpha, const float* src, float* dst,
                  int64_t stride, int64_t offset);
/* TNNCuda.addvv / subvv / mulvv / fmavv (nncuda.pas:120-123):
 * dst[i*incc] = src1[i*inca] op src2[i*incb] (offsets in elements); fmavv:
 * src1*src2 rounded, then + src3 rounded (no fused multiply-add, as the CPU
 * sfmavss).  The increments are taken as they come, as the reference's
 * kernels take them: a negative one walks downward from the pointer + offset
 * (which then names the operand's highest element), 0 reads one element N
 * times.  fmavss (nncuda.pas:137): dst = src*scalar + bias over N
 * contiguous elements at offset.  inverseSqrt (nncuda.pas:151):
 * dst = 1/sqrt(max(src, 1e-6)) strided; alpha unused (as the reference). */
int tns_hip_addvv(tns_ctx* ctx, int64_t N, const float* src1, int64_t src1Offset, int64_t inca,
                  const float* src2, int64_t src2Offset, int64_t incb, float* dst,
                  int64_t dstOffset, int64_t incc);
int tns_hip_subvv(tns_ctx* ctx, int64_t N, const float* src1, int64_t src1Offset, int64_t inca,
                  const float* src2, int64_t src2Offset, int64_t incb, float* dst,
                  int64_t dstOffset, int64_t incc);
int tns_hip_mulvv(tns_ctx* ctx, int64_t N, const float* src1, int64_t src1Offset, int64_t inca,
                  const float* src2, int64_t src2Offset, int64_t incb, float* dst,
                  int64_t dstOffset, int64_t incc);
int tns_hip_fmavv(tns_ctx* ctx, int64_t N, const float* src1, int64_t src1Offset, int64_t inca,
                  const float* src2, int64_t src2Offset, int64_t incb, const float* src3,
                  int64_t src3Offset, int64_t incc, float* dst, int64_t dstOffset,
                  int64_t incd);
int tns_hip_fmavss(tns_ctx* ctx, int64_t N, const float* src, int64_t offset, float scalar,
                   float bias, float* dst);
int tns_hip_inverse_sqrt(tns_ctx* ctx, int64_t N, float alpha, const float* src, float* dst,
                         int64_t stride, int64_t offset);

/* ---- non-convolutional YOLOv3 layers (forward) ------------------------- */
/* TAddLayer.forward (naddlayer.pas:667-720), single input of equal size:
 * out = activate(a + b) (addvv, then the layer's activation). */
int tns_hip_shortcut(tns_ctx* ctx, int64_t N, const float* a, int64_t aOffset, const float* b,
                     int64_t bOffset, float* out, int64_t outOffset, int32_t activation);
/* TNNCuda.upSample (nncuda.pas:136, 1267-1286; CPU upsample()
 * nupsamplelayer.pas:83-113).  outHeight/outWidth are the SMALL tensor's
 * height and width (the reference's naming); planes = aBatch*aChannels.
 * isForward != 0: out[(p*H*s + y)*W*s + x] = scale * in[(p*H + y div s)*W + x div s].
 * isForward == 0: in[...] += scale*out[...] over each input pixel's s x s
 * outputs in the CPU loop order (row outer), deterministic; zeroIn != 0
 * starts from 0 (the reverse layer's output.fill(0)). */
int tns_hip_upsample(tns_ctx* ctx, int64_t aBatch, int64_t aChannels, int64_t outHeight,
                     int64_t outWidth, float* in, int64_t stride, int32_t isForward, float scale,
                     float* out, int32_t zeroIn);
/* TYoloLayer.forward inference part (nyololayer.pas:786-825): out = in with
 * the logistic applied to entries 0, 1 and 4 .. 4+classes of every anchor;
 * data [batch][anchors][classes+5][hw].  (Route/concat = tns_hip_copy of
 * whole tensors, TTensor.concat ntensors.pas:12045-12061.) */
int tns_hip_yolo_forward(tns_ctx* ctx, int64_t batch, int64_t anchors, int64_t classes,
                         int64_t hw, const float* in, float* out);
/* TYoloLayer.forward training part (nyololayer.pas:835-1003: processBatch
 * 500-774, deltaBox 124-202, deltaClass 204-251, averageDeltas 253-269) for
 * one layer, on the device, bit for bit the CPU loop's delta and cost.
 * output [batch][anchors][classes+5][h*w] is what tns_hip_yolo_forward left;
 * truth [batch][maxBoxes][6] on the device, rows x, y, w, h, class, track_id,
 * a row with x == 0 ends an image's list; mask (anchors entries) and biases
 * (2*total floats) are HOST arrays, copied before the call returns.  Writes
 * delta (same shape as output, every element: delta.fill(0) is part of the
 * call), cost[0] = delta.sumSquares() (TTensor.sumSqr, ntensors.pas:9333-9341,
 * the ascending single chain), stats[2*b] = count and stats[2*b+1] = tot_iou
 * of image b (stats may be null), and adds to counters[0] = net.totalBBox and
 * counters[1] = net.rewrittenBBox (device int64).  A NaN or infinite
 * objectness in output is set to 0 where the reference does (an image with at
 * least one truth of a valid class).  Built: iou_loss=mse, iou_thresh_kind=iou,
 * scale_x_y=1; not built: focal_loss, objectness_smooth, label_smooth_eps,
 * new_coords, counters_per_class, map, embedding_layer, [net] adversarial and
 * the bad-label rejection block (896-990); the GIoU/DIoU/CIoU statistics,
 * avg_* / recall, labels and classIds are not computed.  Departure: a truth
 * whose cell trunc(x*w), trunc(y*h) lies outside the grid is skipped in the
 * truth pass (the reference writes out of bounds).  TNS_ERR_ARG, before
 * anything is launched or written: a negative size, netW / netH below 1, a
 * null operand (stats excepted), a mask entry outside [0, total), maxBoxes
 * outside [1, 2048], anchors or total above 32, batch above 65535, a buffer
 * beyond 2^31 elements. */
int tns_hip_yolo_loss(tns_ctx* ctx, int64_t batch, int64_t anchors, int64_t classes, int64_t h,
                      int64_t w, int64_t total, const int64_t* mask, const float* biases,
                      int64_t maxBoxes, int64_t netW, int64_t netH, float ignoreThresh,
                      float truthThresh, float iouThresh, float iouNormalizer,
                      float objNormalizer, float* output, const float* truth, float* delta,
                      float* cost, float* stats, int64_t* counters);
/* TNNet.Detections' per-layer part (nnet.pas:584-677): TYoloLayer.
 * getDetectionCount + getDetections + correctBoxes (nyololayer.pas:378-498,
 * getBox 105-122, not newCoords) for one layer and all images, bit for bit the
 * CPU loop's rows.  output [batch][anchors][classes+5][h*w] is what
 * tns_hip_yolo_forward left; mask (anchors entries) and biases (2*total
 * floats) are HOST arrays, copied before the call returns; every other
 * operand is on the device: counts int64[batch], boxes [batch][capacity][4]
 * (x, y, w, h), objectness [batch][capacity], probs [batch][capacity][classes].
 * A candidate (cell i, anchor a) is taken when its objectness is > thresh
 * (strict; NaN is not taken: the reference's NaN check is commented out,
 * lines 392-394, 424-426).  The taken candidates of image b become the rows
 * counts[b], counts[b]+1, ... in the reference's order, cell i outer, anchor a
 * inner: bbox = getBox(mask[a], .., col, row, netW, netH, h*w) after
 * correctBoxes(imW, imH, netW, netH, relative, letter); objectness; prob[j] =
 * objectness * class_j where that product is > thresh, else 0 (435-443).
 * counts[b] then grows by the number of taken candidates, whether their rows
 * fitted or not: rows at or beyond capacity are not written, and counts[b] >
 * capacity afterwards is how the caller learns of it (the reference's count
 * pass and fill pass in one).  So the layers of a network append into one
 * buffer when called in network order on counts zeroed once.  Nothing outside
 * the taken rows is written.  Not built: new_coords, the embedding output,
 * TRegionLayer.  A letterbox whose scaled extent truncates to 0 divides by
 * zero as the reference does; the result is then IEEE's, not an exception.
 * TNS_ERR_ARG, before anything is launched or written: a negative size; netW,
 * netH, imW or imH below 1 or above 2^24; a null operand where there is work
 * (batch, anchors and h*w all above 0); a mask entry outside [0, total);
 * anchors or total above 32; capacity outside [1, 4194304]; batch above 65535;
 * a buffer beyond 2^31 elements.  batch == 0 is a successful no-op. */
int tns_hip_yolo_detections(tns_ctx* ctx, int64_t batch, int64_t anchors, int64_t classes,
                            int64_t h, int64_t w, int64_t total, const int64_t* mask,
                            const float* biases, int64_t netW, int64_t netH, int64_t imW,
                            int64_t imH, float thresh, int32_t relative, int32_t letter,
                            const float* output, int64_t capacity, int64_t* counts, float* boxes,
                            float* objectness, float* probs);
/* TDetections.doNMSSort (ntypes.pas:1612-1649, Comparer 1554-1565, TBox.iou
 * 1059-1108 in singles) on the rows tns_hip_yolo_detections left, in place on
 * probs.  For image b the rows 0 .. min(counts[b], capacity)-1 whose
 * objectness is not 0 take part (the reference swaps the zero-objectness rows
 * out of `total`, 1619-1633).  For each class k on its own: the rows in order
 * of prob[k] descending; a row whose prob[k] is still non-zero when the walk
 * reaches it sets prob[k] of every later row to 0 whose bbox has an iou with
 * it > thresh; a row already zeroed suppresses nothing.  Departures: (1) rows
 * keep their place (the reference leaves the array permuted in the last
 * class's sort order); per row the result is the same.  (2) Equal non-zero
 * scores order the lower row first; the reference's QuickSort is not stable,
 * so their order there is unspecified (ties at zero do not matter: a zero row
 * suppresses nothing and zeroing it changes nothing).  NaN scores order by
 * their bit pattern, above +Inf when positive.  Only prob entries that become
 * 0 are written.  Any number of non-zero rows per class up to capacity:
 * up to 2048 of one (image, class) are sorted on chip, more are walked by
 * repeated selection with the same result.  doNMSObj and the DIoU / corners
 * NMS kinds are not built.  TNS_ERR_ARG, before anything is launched or
 * written: a negative size, capacity outside [1, 4194304], batch above 65535,
 * a buffer beyond 2^31 elements, a null operand where there is work (batch
 * and classes above 0).  batch == 0, or all counts 0, is a successful no-op. */
int tns_hip_nms_sort(tns_ctx* ctx, int64_t batch, int64_t capacity, int64_t classes,
                     const int64_t* counts, const float* boxes, const float* objectness,
                     float* probs, float thresh);

/* ---- image preprocessing (TImageData, ntypes.pas:837-947; image.hip) ----
 * TImageData.resize, or with letter != 0 letterBox / letterBoxEx (resize,
 * fill 0.5, Embed), of `count` images of differing sizes into the network
 * input dst [count][channels][netH][netW] on the device, in one launch a
 * batch, bit for bit the reference's values; every element of dst is written.
 * Sources: interleaved bytes as decoders deliver them (h rows of w pixels,
 * pixelStride bytes a pixel with channel k at byte k, rowStride bytes a row),
 * or planar floats, TImageData's own layout ([channels][h] rows of w floats,
 * rowStride floats a row, so a plane is h*rowStride floats).  src is a device
 * pointer; geom is a HOST array int64[count][4] = {offset, w, h, rowStride}
 * per image, offset the image's first element from src (bytes, or floats),
 * copied before the call returns.  placed, optional, is a HOST array
 * int64[count][4] that receives {new_w, new_h, dx, dy} per image: the resize
 * target and where it sits in the net input.  Without letter that is {netW,
 * netH, 0, 0}.  With letter: if netW*h < netH*w (the exact form of (aWidth /
 * self.w) < (aHeight / self.h)) new_w = netW, new_h = (h*netW) div w, else
 * new_h = netH, new_w = (w*netH) div h; dx = (netW-new_w) div 2, dy likewise;
 * every pixel outside the rectangle is 0.5.  (letterBoxEx's ratio is
 * single(netW/w) in the first branch, single(netH/h) in the other: the caller
 * has both operands.)
 * The resize, for target pixel (x, r), channel k, in singles with every
 * product and sum rounded and no FMA: w_scale = single((w-1)/(new_w-1)),
 * h_scale likewise; P(y) = src(w-1, y) if x = new_w-1 or w = 1, else
 * (1-dx)*src(ix, y) + dx*src(ix+1, y) with sx = x*w_scale, ix = trunc(sx),
 * dx = sx-ix; then sy = r*h_scale, iy = trunc(sy), dy = sy-iy, val =
 * (1-dy)*P(iy), and unless r = new_h-1 or h = 1, val += dy*P(iy+1).  The last
 * row is not special-cased as the last column is: where single(new_h-1)*
 * h_scale rounds below h-1 (16 -> 416 rows, 479 -> 416, ...) it is
 * (1-dy)*P(h-2) with dy just below 1, a near-black row, as in the reference.
 * A byte b becomes a float through a 256-entry table, tableKind 0:
 * single((b*257)/65280), the FPC loader's TFPColor word over $ff00
 * (ntypes.pas:749-752; 255 maps above 1); 1: single(b/255), the Delphi
 * loader's (716-718); 2: table, a HOST array of 256 floats, copied before the
 * call returns.
 * Both entries join a pending dW of the pipelined conv backward on every
 * call (they write the network input, which that dW reads).
 * TNS_ERR_ARG, before anything is launched or written: a null operand where
 * count > 0 (src, geom, dst; table under tableKind 2); count outside [0,
 * 2^20]; channels outside 1..4 for bytes (1..1024 for floats); pixelStride <
 * channels or above 32768; tableKind outside 0..2; a negative offset; a rowStride shorter
 * than a row; w, h, netW or netH outside [1, 32768]; a resize target (netW x
 * netH, or new_w x new_h) below 2 either way, where the reference divides by
 * zero.  count == 0 is a successful no-op. */
int tns_image_bytes_to_input(tns_ctx* ctx, int64_t count, const uint8_t* src, const int64_t* geom,
                             int64_t channels, int64_t pixelStride, int32_t tableKind,
                             const float* table, int64_t netW, int64_t netH, int32_t letter,
                             float* dst, int64_t* placed);
int tns_image_floats_to_input(tns_ctx* ctx, int64_t count, const float* src, const int64_t* geom,
                              int64_t channels, int64_t netW, int64_t netH, int32_t letter,
                              float* dst, int64_t* placed);

/* ---- max / local-average pooling (TMaxPoolLayer, nMaxPoolLayer.pas) ----- */
/* Geometry, shared by the four entries: input [aBatch][c][h][w], output
 * [aBatch][outC][outH][outW] with outC == c, outH == (h + padding -
 * kernelSize) div stride_y + 1 and outW likewise with stride_x
 * (nMaxPoolLayer.pas:107-109).  Window (i, j) covers rows off + i*stride_y ..
 * + kernelSize - 1 and columns off + j*stride_x .. + kernelSize - 1, off =
 * -(padding div 2); taps outside the input do not take part.  TNS_ERR_ARG,
 * before anything is launched or written: a negative size, kernelSize or a
 * stride below 1, negative padding, outC != c, an output shape other than the
 * one above, kernelSize beyond the padded input, a plane beyond 2^31 elements,
 * a null operand where there is work.  maxpool_depth and antialiasing are not
 * built (the reference's device path has neither).
 *
 * tns_hip_maxpool_forward = TNNCuda.forwardMaxPool (nncuda.pas:132), the CPU
 * loop nMaxPoolLayer.pas:415-451: the window is scanned rows outer, columns
 * inner, from max = -FLT_MAX, max_i = -1, with a strict `val > max`: the first
 * maximum in scan order wins, NaN and -inf are never taken, and a window with
 * nothing above -FLT_MAX gives output -FLT_MAX and index -1.  indexes[out] is
 * the maximum's element index in the whole input buffer (cur_w + w*(cur_h +
 * h*(k + b*c))), int64 (TSizeIntTensor); indexes may be null (inference):
 * only output is written then.
 *
 * tns_hip_maxpool_backward = TNNCuda.backwardMaxPool (nncuda.pas:133) plus the
 * layer's geometry, which the ordered form needs: output (state.delta, the
 * layer below's delta, [aBatch][outC][h][w]) gets, per element, the delta of
 * every output whose stored index names it, added one rounding at a time in
 * ascending output index — the CPU loop's order (nMaxPoolLayer.pas:501-513).
 * The reference's device kernel scatters `output[index] += delta[id]`
 * without atomics, a race wherever stride < kernelSize; here one thread owns
 * an input element and gathers, so the result is deterministic and the CPU's.
 * Departure: an index of -1 names no element and is ignored (the reference
 * reads and writes state.delta[-1], out of bounds).  Elements that no index
 * names keep their bits (nothing is added to them; a 16-byte group without a
 * named element is not written at all).
 *
 * tns_hip_avgpool_forward / _backward: TMaxPoolLayer.forwardAvgPool /
 * backwardAvgPool (nMaxPoolLayer.pas:465-499, 515-542), which the reference
 * runs on the CPU only (its GPU branch does nothing for avg pooling).
 * Forward: the in-range taps summed in scan order, then one division by
 * their count.  Backward: state.delta[p] += delta[out] / float(kernelSize *
 * kernelSize) for every window covering p, in ascending output index — the
 * reference divides by kernelSize^2 here, not by the in-range count.  Also
 * TNS_ERR_ARG: a geometry in which some window has no tap inside the input
 * (a zero counter in the reference). */
int tns_hip_maxpool_forward(tns_ctx* ctx, int64_t aBatch, int64_t outC, int64_t outH,
                            int64_t outW, const float* input, int64_t c, int64_t h, int64_t w,
                            int64_t stride_x, int64_t stride_y, int64_t padding,
                            int64_t kernelSize, int64_t* indexes, float* output);
int tns_hip_maxpool_backward(tns_ctx* ctx, int64_t aBatch, int64_t outC, int64_t outH,
                             int64_t outW, float* output, const int64_t* indexes,
                             const float* delta, int64_t h, int64_t w, int64_t stride_x,
                             int64_t stride_y, int64_t padding, int64_t kernelSize);
int tns_hip_avgpool_forward(tns_ctx* ctx, int64_t aBatch, int64_t outC, int64_t outH,
                            int64_t outW, const float* input, int64_t c, int64_t h, int64_t w,
                            int64_t stride_x, int64_t stride_y, int64_t padding,
                            int64_t kernelSize, float* output);
int tns_hip_avgpool_backward(tns_ctx* ctx, int64_t aBatch, int64_t outC, int64_t outH,
                             int64_t outW, float* output, const float* delta, int64_t h,
                             int64_t w, int64_t stride_x, int64_t stride_y, int64_t padding,
                             int64_t kernelSize);

/* ---- global average pooling (TAvgPoolLayer, navgpoollayer.pas) ---------- */
/* The layer every darknet classifier ends in ([avgpool]; parseAvgPool,
 * nparser.pas:294-299): input [aBatch][c][h][w] -> output [aBatch][c].  Here
 * the data is [planes][n], planes = aBatch*c, n = h*w, planes contiguous.
 * TNNCuda has no such method — the reference runs this layer on the CPU — so
 * the two entries carry no tns_hip_ prefix and, like the tns_image_* entries,
 * join a pending dW of the pipelined conv backward on every call instead of
 * taking a place in the hazard table.
 *
 * tns_pool_global_avg_forward = TAvgPoolLayer.forward (navgpoollayer.pas:
 * 60-84): output[p] = Sum(plane p) / n.  Sum is vssum_avx2 (ntensors.pas:
 * 3592-3620): eight accumulators from +0, accumulator j adding elements j,
 * j+8, j+16, ... of the first 8*(n div 8) in that order; s_j = a_j + a_(j+4)
 * for j < 4; (s0+s1) + (s2+s3); the n mod 8 tail elements added one at a time
 * in index order; then one division by float(n).  Every step is one float32
 * rounding (a plane of -0.0 gives +0.0: the accumulators start at +0).  Eight
 * lanes own a plane, the two folds run across lanes; a very large plane is a
 * long sequential chain per lane, the price of the order.
 *
 * tns_pool_global_avg_backward = TAvgPoolLayer.backward (navgpoollayer.pas:
 * 86-108): stateDelta[p*n + i] += delta[p] / float(n) for every i: the
 * quotient rounded once, then one add per element (16-byte accesses between
 * the buffer's first and last 16-byte boundary, single elements outside).
 *
 * Departures: the reference converts n to the quotient's type at each use;
 * here float(n) must be exact, so n > 2^24 is refused.  TNS_ERR_ARG, before
 * anything is launched or written: a negative size; n > 2^24; planes*n beyond
 * 2^63 bytes (the other pool entries' bound); a null operand where there is
 * work; output or stateDelta overlapping the other operand.  planes == 0 or
 * n == 0 does nothing and returns TNS_OK. */
int tns_pool_global_avg_forward(tns_ctx* ctx, int64_t planes, int64_t n, const float* input,
                                float* output);
int tns_pool_global_avg_backward(tns_ctx* ctx, int64_t planes, int64_t n, const float* delta,
                                 float* stateDelta);

/* ---- dropout and the elementwise loss heads (heads.hip) ----
 * tns_hip_dropout_forward = TNNCuda.forwardDropout, the reference's device
 * kernel (cuda_sgemm.cu:1617-1645), a pure function of (seed, i) — the CPU
 * layer draws from Pascal's random(), which cannot be reproduced.  Per
 * element i (a 64-bit index):
 *   x = uint64(seed) + i           (seed in [0, 2^32); the sum does not wrap)
 *   x ^= x >> 12; x ^= x << 25; x ^= x >> 27; x *= 0x2545F4914F6CDD1D
 *   rnd[i] = float(x mod 2^28) / 2^28     (conversion to nearest even)
 *   dst[i] = rnd[i] < probability ? +0.0f : src[i] * scale
 * A dropped element is +0.0f whatever src held (NaN, Inf included).
 * tns_hip_dropout_backward (cuda_sgemm.cu:1647-1653) is the same select over
 * the stored rnd.  Both work in place: src == dst is how the reference calls
 * them (ndropoutlayer.pas:162, 170).  TNS_ERR_ARG, before any launch: N < 0,
 * seed outside [0, 2^32), a null operand with N > 0, rnd overlapping src or
 * dst, src and dst overlapping other than exactly.  N == 0 does nothing.
 *
 * tns_hip_cost_l2 = TNNCuda.costL2 (cuda_sgemm.cu:1655-1662): r = truth -
 * pred; delta = r; error = r * r, each one rounding.
 *
 * tns_hip_cross_entropy_logistic = TNNCuda.crossEntropyLogistic, the CPU
 * statement (nlogisticlayer.pas:72-77): delta = t - p; error = -t*ln(max(p,
 * eps)) - (1-t)*ln(max(1-p, eps)), eps = 1e-6f; max, 1-p and 1-t in float,
 * the logs, products and subtraction in double, rounded once to float. */
int tns_hip_dropout_forward(tns_ctx* ctx, int64_t N, int64_t seed, float probability,
                            float scale, const float* src, float* rnd, float* dst);
int tns_hip_dropout_backward(tns_ctx* ctx, int64_t N, float probability, float scale,
                             const float* src, const float* rnd, float* dst);
int tns_hip_cost_l2(tns_ctx* ctx, int64_t N, const float* pred, const float* truth,
                    float* delta, float* error);
int tns_hip_cross_entropy_logistic(tns_ctx* ctx, int64_t N, const float* pred,
                                   const float* truth, float* delta, float* error);

/* ---- the gate stage of one LSTM time step (lstm.hip) ----
 * Backend-specific fused entries (TNNCuda has none): what
 * TLSTMLayer.forwardGPU / backwardGPU (nlstmlayer.pas:933-973, 1046-1255)
 * issue as addvv / ActivateArray / mulvv / fmavv / copy / DeriveArray calls
 * around the eight connected sub-layers, per element k of the step's N =
 * streams * outputs floats.  w_x / u_x are the step's slice of the sub-layers'
 * output; a_x = w_x[k] + u_x[k].  Every written operation is one float32
 * rounding; logistic = 1/(1+exp(-x)) in double rounded once, tanh =
 * (px-nx)/(px+nx) on the single-rounded exponentials.
 * tns_hip_lstm_gates_forward:
 *   f = logistic(a_f)  i = logistic(a_i)  g = tanh(a_g)  o = logistic(a_o)
 *   t = i*g;  c = c_state[k]*f;  c = c + t;  h = tanh(c)*o
 *   c -> c_state[k], cell_slice[k];  h -> h_state[k], out_slice[k]
 * tns_hip_lstm_gates_backward (f, i, g, o as above):
 *   t = tanh(cell_i[k]);  d = delta_i[k]
 *   e = d*o;  e = e*(1 - t*t);  e = dc[k] + e
 *   do = (d*t)*((1-o)*o)      dg = (e*i)*(1 - g*g)
 *   di = (e*g)*((1-i)*i)      df = (e*cprev[k])*((1-f)*f)
 *   dc[k] = e*f
 * Each gate delta is stored clamped to [-1, 1] (v < -1 ? -1 : v > 1 ? 1 : v;
 * a NaN stays) — the clamp(delta, 1) that opens the sub-layer's backwardGPU
 * (nconnectedlayer.pas:771) — to the w-side slice dw_x and, where du_x is not
 * null, to the u-side slice.  dc is not clamped.  c_state and dc are read and
 * written in place.  TNS_ERR_ARG, before any launch and with every output
 * untouched: N < 0, a null operand with N > 0 (du_x excepted), an output
 * (c_state, h_state, cell_slice, out_slice; dc, dw_x, du_x) overlapping any
 * other operand.  Inputs may overlap one another.  N == 0 does nothing. */
int tns_hip_lstm_gates_forward(tns_ctx* ctx, int64_t N, const float* wf, const float* wi,
                               const float* wg, const float* wo, const float* uf,
                               const float* ui, const float* ug, const float* uo,
                               float* c_state, float* h_state, float* cell_slice,
                               float* out_slice);
int tns_hip_lstm_gates_backward(tns_ctx* ctx, int64_t N, const float* wf, const float* wi,
                                const float* wg, const float* wo, const float* uf,
                                const float* ui, const float* ug, const float* uo,
                                const float* cell_i, const float* cprev, const float* delta_i,
                                float* dc, float* dwf, float* dwi, float* dwg, float* dwo,
                                float* duf, float* dui, float* dug, float* duo);

/* ---- the elementwise stage of one RNN time step (rnn.hip) ----
 * Backend-specific fused entries (TNNCuda has none): what
 * TRNNLayer.rnnStepForward / rnnStepBackward (nrnnlayer.pas:148-216) and the
 * head of its connected sub-layers' forward / backward (nconnectedlayer.pas:
 * 157-322) issue as forwardBias, ActivateArray, fill / copy, addvv, clamp,
 * DeriveArray and copy calls, per element k of the step's N = streams * H
 * floats.  Every written operation is one float32 rounding; act / grad are
 * ActivateArray's / DeriveArray's formulas.
 * tns_hip_rnn_state_forward (in_slice / self_slice: the step's slice of the
 * input and self sub-layers' output, the NT product only):
 *   a = in_slice[k];    a = a + in_bias[k % H];    a = act(a, in_act)
 *   b = self_slice[k];  b = b + self_bias[k % H];  b = act(b, self_act)
 *   s = (state_prev ? state_prev[k] : 0.0f) + a;   s = s + b
 *   a -> in_slice[k];  b -> self_slice[k];  s -> state_next[k]
 * A null bias skips that add (the slice is normalized and biased already:
 * batch norm).  0.0f + a is evaluated (the reference's fill, then add), so
 * a = b = -0 stores +0.  state_prev may be null (no shortcut) or state_next
 * itself (inference, where the step writes the slice it reads).
 * tns_hip_rnn_delta_backward:
 *   d = clamp1(delta[k]) * grad(out[k], act);     d -> delta[k]
 *   delta2[k] = clamp1(d) * grad(out2[k], act2)   (delta2 not null)
 * clamp1(v) = v < -1 ? -1 : v > 1 ? 1 : v (a NaN stays): the clamp(delta, 1)
 * + DeriveArray that open a sub-layer's backward, on one slice; with delta2
 * also the copy into the input sub-layer's delta and that sub-layer's clamp +
 * DeriveArray (valid when the self sub-layer is not batch-normalized).
 * TNS_ERR_ARG, before any launch and with every output untouched: N < 0,
 * H < 1, a null operand with N > 0 (the biases, state_prev and delta2 / out2
 * without delta2 excepted), an output (in_slice, self_slice, state_next;
 * delta, delta2) overlapping any other operand — state_prev == state_next is
 * one operand.  TNS_ERR_UNSUPPORTED: an activation ActivateArray rejects.
 * Inputs may overlap one another.  N == 0 does nothing. */
int tns_hip_rnn_state_forward(tns_ctx* ctx, int64_t N, int64_t H, float* in_slice,
                              const float* in_bias, int32_t in_act, float* self_slice,
                              const float* self_bias, int32_t self_act,
                              const float* state_prev, float* state_next);
int tns_hip_rnn_delta_backward(tns_ctx* ctx, int64_t N, float* delta, const float* out,
                               int32_t act, float* delta2, const float* out2, int32_t act2);

/* ---- batch norm / softmax (TNNCuda twins, nncuda.pas:1056-1510; CPU
 * semantics ntensors.pas:7687-7830, 8693-8951, 9102-9177,
 * nsoftmaxlayer.pas:83-137).  Data is [groups][channels][blockSize]. ---- */
/* meansAndVars: blockSize = srcSize/(dstSize*groups); unbiased variance */
int tns_hip_means_and_vars(tns_ctx* ctx, int64_t srcSize, int64_t dstSize, int64_t groups,
                           const float* src, int64_t offset, float* means, float* vars);
/* TNNCuda.means / TNNCuda.variances — nncuda.pas:1330-1369, the pair the
 * reference's batchNormGPU (nbaselayer.pas:583-584) and
 * TConnectedLayer.forwardGPU (nconnectedlayer.pas:664-665) call.  Same
 * blockSize and results as the two halves of tns_hip_means_and_vars (CPU
 * MeansAndVars order, ntensors.pas:9102-9177: vssum_avx2 lanes per block for
 * the mean, srss lanes about the GIVEN means for the unbiased variance,
 * TNS_OPT_SRSS_QUIRK applying to the latter). */
int tns_hip_means(tns_ctx* ctx, int64_t srcSize, int64_t dstSize, int64_t groups,
                  const float* src, int64_t offset, float* means);
int tns_hip_variances(tns_ctx* ctx, int64_t srcSize, int64_t dstSize, int64_t groups,
                      const float* src, int64_t offset, const float* means, float* vars);
/* normalize: blockSize = dstSize/(srcSize*groups); bs==1: (x-m)/sqrt(max(v,eps)),
 * bs>1: (x-m)/max(sqrt(v),eps) */
int tns_hip_normalize(tns_ctx* ctx, int64_t srcSize, int64_t dstSize, int64_t groups,
                      const float* means, int64_t meansStride, const float* vars,
                      int64_t varsStride, float* dst, int64_t dstOffset);
/* forwardScale / forwardScaleAdd: dst[(b*S+i)*bs+j] = dst*scale[i*incb] (+ bias[i*incb]) */
int tns_hip_forward_scale(tns_ctx* ctx, int64_t dstSize, float* dst, int64_t offset,
                          int64_t scaleSize, const float* scale, int64_t incb, int64_t batch);
int tns_hip_forward_scale_add(tns_ctx* ctx, int64_t dstSize, float* dst, int64_t offset,
                              int64_t scaleSize, const float* scales, const float* biases,
                              int64_t incb, int64_t batch);
/* meansAndVarsDelta / normalizeDelta (sMeanAndVarianceDelta / sNormalizeDelta) */
int tns_hip_means_and_vars_delta(tns_ctx* ctx, int64_t srcSize, int64_t dstSize, int64_t groups,
                                 const float* delta, const float* x, int64_t offset,
                                 const float* mean, const float* variance, float* mean_delta,
                                 float* variance_delta);
int tns_hip_normalize_delta(tns_ctx* ctx, int64_t deltaSize, int64_t meanSize, int64_t groups,
                            float* delta, const float* x, int64_t offset, const float* mean,
                            const float* variance, const float* mean_delta,
                            const float* variance_delta);
/* addDots: dst[i] += sum x_norm*delta over (group, block) */
int tns_hip_add_dots(tns_ctx* ctx, int64_t N, int64_t dstSize, int64_t groups,
                     const float* src1, const float* src2, int64_t srcOffset, float* dst);
/* TSoftmaxLayer.softmaxBatch / softmaxCrossEntropy.  softmaxBatch: for every
 * (b, g), softmax over the N elements every `stride` from
 * b*batch_size + g*group_size; stride >= 1, the counts and sizes >= 0
 * (TNS_ERR_ARG otherwise). */
int tns_hip_softmax_batch(tns_ctx* ctx, int64_t N, const float* input, int64_t iOffset,
                          int64_t batch, int64_t batch_size, int64_t groups, int64_t group_size,
                          int64_t stride, float temp, float* output, int64_t oOffset);
int tns_hip_cross_entropy_softmax(tns_ctx* ctx, int64_t N, const float* pred, const float* truth,
                                  float* delta, float* error);
/* TTensor.Sum in the vssum_avx2 order (cost), result written to *out (device) */
int tns_hip_sum(tns_ctx* ctx, int64_t N, const float* src, int64_t offset, float* out);

/* ---- fused connected-network train step (BASELINE config 5) ------------
 * One TNNet.Propagate + TNNet.update (nnet.pas:275-450) for nlayers
 * TConnectedLayer (widths[l] -> widths[l+1], activation acts[l], batch norm
 * when bn != 0) followed by a TSoftmaxLayer, as ONE kernel launch.  buf holds
 * the packed parameters and state (layout: oracle/tns_oracle.h
 * ora_mlp_train_step), sized tns_mlp_buffer_floats().  *cost (device) gets
 * the softmax layer's loss.Sum().  Limits: nlayers <= 32,
 * 9*batch*max(widths[1..]) <= 40960 (one CU's LDS). */
int64_t tns_mlp_buffer_floats(int32_t nlayers, const int64_t* widths, int32_t bn, int64_t batch);
int tns_hip_mlp_train_step(tns_ctx* ctx, int32_t nlayers, const int64_t* widths,
                           const int32_t* acts, int32_t bn, int64_t batch, const float* X,
                           const float* truth, float learningRate, float momentum, float decay,
                           float* buf, float* cost);

/* ---- layer drivers (host logic of the reference, running on device) ---- */

/* TTensor.Conv2D — ntensors.pas:8252-8349.  input: batch x C x H x W,
 * weights: filters x (C*kH*kW) row-major, out: batch x filters x oH x oW.
 * im2col is skipped for 1x1 / stride 1 / dilation 1 (ntensors.pas:8286-8312).
 * workspace: >= batch*C*kH*kW*oH*oW floats, or NULL to use ctx scratch.
 * NOTE: mirrors the reference's slot swap: xDilation is passed as dilationY
 * (ntensors.pas:8303); harmless for square dilation.  With xDilation !=
 * yDilation the swapped im2col's column grid differs from the oH x oW the col
 * buffer and the GEMM are sized for (the reference overruns its workspace
 * there): TNS_ERR_UNSUPPORTED, the message naming both sizes, before anything
 * is allocated or launched; out is left untouched. */
int tns_hip_conv2d(tns_ctx* ctx, int64_t batch, int64_t C, int64_t H, int64_t W,
                   const float* input, const float* weights, int64_t filters,
                   int64_t kH, int64_t kW, int64_t wPadding, int64_t hPadding,
                   int64_t xStride, int64_t yStride, int64_t xDilation, int64_t yDilation,
                   float* workspace, float* out);

/* TConvolutionalLayer.forward / forwardGPU with fused (folded) BN —
 * nConvolutionLayer.pas:457-569 / 1022-1153: Conv2D -> forwardBias ->
 * activate.  fused selects the schedule (same arithmetic, same bits, in all):
 *   TNS_CONV_UNFUSED  (0) the three reference stages (im2col, GEMM, bias+act)
 *   TNS_CONV_FUSED    (1) library's choice among the two below
 *   TNS_CONV_IM2COL   (2) im2col into workspace + SGEMM with bias+act epilogue
 *   TNS_CONV_IMPLICIT (3) implicit GEMM: the SGEMM gathers its B tiles from
 *                         the image (no col matrix, workspace unused); a
 *                         3-channel 3x3 layer with 16 or 32 filters runs the
 *                         direct kernel instead (same fmaf chains) */
enum { TNS_CONV_UNFUSED = 0, TNS_CONV_FUSED = 1, TNS_CONV_IM2COL = 2, TNS_CONV_IMPLICIT = 3 };
int tns_hip_conv_forward(tns_ctx* ctx, int64_t batch, int64_t C, int64_t H, int64_t W,
                         const float* input, const float* weights, const float* biases,
                         int64_t filters, int64_t kSize, int64_t stride, int64_t padding,
                         int64_t dilation, int32_t activation, float* workspace,
                         float* out, int32_t fused);

/* TConvolutionalLayer.forward in TRAINING with batch norm (nConvolutionLayer.
 * pas:457-569 -> TBaseLayer.batchNorm, nbaselayer.pas:336-370): Conv2D into
 * out; training != 0: MeansAndVars -> mean/variance, rolling_mean/variance
 * *= (1 - bnMomentum) then += bnMomentum*stat (axpy), x := out,
 * blockNormalize, x_norm := out; training == 0: blockNormalize with the
 * rolling statistics; then forwardScale(scales), forwardBias(biases),
 * activate.  Tensors [batch][filters][oH*oW]; statistics per filter.  The
 * layer's bnMomentum is 0.1 (nbaselayer.pas:188).  In-place and
 * bit-exact against the reference order (one fused pass after the stats). */
int tns_hip_conv_forward_train(tns_ctx* ctx, int64_t batch, int64_t C, int64_t H, int64_t W,
                               const float* input, const float* weights, int64_t filters,
                               int64_t kSize, int64_t stride, int64_t padding, int64_t dilation,
                               int32_t activation, const float* scales, const float* biases,
                               float* rolling_mean, float* rolling_variance, float bnMomentum,
                               int32_t training, float* mean, float* variance, float* x,
                               float* x_norm, float* workspace, float* out);

/* TConvolutionalLayer.backward without batch-norm (nConvolutionLayer.pas:
 * 571-671): delta *= f'(output) (Derivative), bias_updates += addSums(delta),
 * im2col(input), weight_updates += delta_b . col_b^T per image (NT, beta 1),
 * and if state_delta != NULL: col = W^T . delta (TN strided batched, beta 0)
 * then col2im accumulates into state_delta.  delta is updated in place.
 * workspace (batch*C*k*k*outH*outW floats) may be NULL (context scratch).
 * The backward im2col / col2im pad with padding*dilation (640, 665); a
 * dilation whose columns differ from the layer's outH x outW (92-100) is
 * refused with TNS_ERR_UNSUPPORTED ("same" paddings work at any dilation).
 * At dilation > 1 this REPRODUCES THE REFERENCE, not the calculus:
 *  - state_delta follows scol2im's input_row := (kernel_row - pad)*dil
 *    (ntensors.pas:11650-11715) with pad = padding*dilation, which is not
 *    the adjoint of im2col — it is not the true input gradient (reference
 *    quirk 3);
 *  - tns_hip_conv_forward(_train) at dilation > 1 writes out_dim(H, padding,
 *    kSize, dilation, stride) columns per filter, while this backward takes
 *    delta / output with the layer's (H + 2*padding - kSize)/stride + 1
 *    (nConvolutionLayer.pas:92-100): the two agree only where those sizes
 *    coincide ("same" paddings), exactly as in the reference. */
int tns_hip_conv_backward(tns_ctx* ctx, int64_t batch, int64_t C, int64_t H, int64_t W,
                          const float* input, const float* weights, int64_t filters,
                          int64_t kSize, int64_t stride, int64_t padding, int64_t dilation,
                          int32_t activation, const float* output, float* delta,
                          float* bias_updates, float* weight_updates, float* workspace,
                          float* state_delta);
/* The same with batch norm (isBatchNormalized, nConvolutionLayer.pas:601-602):
 * batchNormBack (nbaselayer.pas:372-395) replaces the bias term —
 * scale_updates += addDots(x_norm, delta); delta *= scales (forwardScale);
 * MeansAndVarsDelta(delta, x, mean, variance) -> mean_delta / variance_delta;
 * normalizeDelta — then the weight / input gradients as above.  x, x_norm,
 * mean, variance are the forward's (tns_hip_conv_forward_train). */
int tns_hip_conv_backward_bn(tns_ctx* ctx, int64_t batch, int64_t C, int64_t H, int64_t W,
                             const float* input, const float* weights, int64_t filters,
                             int64_t kSize, int64_t stride, int64_t padding, int64_t dilation,
                             int32_t activation, const float* output, float* delta,
                             const float* scales, const float* x, const float* x_norm,
                             const float* mean, const float* variance, float* scale_updates,
                             float* mean_delta, float* variance_delta, float* weight_updates,
                             float* workspace, float* state_delta);

/* ---- several GPUs from ONE process (config 4) ---------------
 * gemmStridedBatched over n devices (devices[i] for slot i; a device may
 * appear twice): HOST pointers, as the op-table gemmStridedBatched
 * (ntensors.pas:348-351), cblas_sgemm semantics.  The batch is split into n
 * contiguous shards (the first batchCount % n one GEMM longer); each slot
 * has its own context, stream and host thread and pipelines its shard's
 * uploads, GEMMs and downloads.  A shared operand (strideA or strideB = 0,
 * the conv weights of nConvolutionLayer.pas:773) crosses PCIe once, to slot
 * 0, and reaches the other devices by peer copies (xGMI).  Results are bit
 * identical to the single-device call.  Returns a status. */
int tns_hip_sgemm_strided_batched_multi(const int32_t* devices, int32_t n, uint8_t transA,
                                        uint8_t transB, int64_t M, int64_t N, int64_t K,
                                        float alpha, const float* A, int64_t lda,
                                        int64_t strideA, const float* B, int64_t ldb,
                                        int64_t strideB, float beta, float* C, int64_t ldc,
                                        int64_t strideC, int64_t batchCount);
/* Spread the op-table drop-ins tns_cblas_sgemm_batch_strided / tns_cblas_sgemm
 * over these devices (n <= 1: the default single context again), so an
 * unmodified Pascal binding drives several GPUs. */
int tns_set_op_devices(const int32_t* devices, int32_t n);

/* ---- telemetry (TTensorMetrics-style per-op device timing) ------------ */
int    tns_hip_set_telemetry(tns_ctx* ctx, int32_t enable);
double tns_hip_op_ms(tns_ctx* ctx, int32_t op);   /* accumulated ms per op */
enum { TNS_OP_GEMM = 0, TNS_OP_IM2COL = 1, TNS_OP_COL2IM = 2, TNS_OP_BIAS = 3,
       TNS_OP_ACTIVATE = 4, TNS_OP_COUNT = 5 };

/* ---- tuning / options -------------------------------------------------- */
/* SGEMM tile-shape variants (the production path picks one per problem;
 * these force one, for sweeps).  variant < 0 = heuristic.  Some shapes are
 * NN-with-aligned-operands only and return TNS_ERR_UNSUPPORTED otherwise. */
int         tns_gemm_variant_count(void);
/* k-major-A conv tiles of the backward's col = W^T . delta (TNS_OPT_DX_TILE = v) */
int         tns_conv_dx_tile_count(void);
/* implicit transposed-convolution forms of the conv backward's state.delta
 * (TNS_OPT_DX_CONV = v) */
int         tns_conv_dx_conv_count(void);
/* residue-sequential dW forms of the conv backward (TNS_OPT_DW_RES = v) */
int         tns_conv_dw_res_count(void);
/* implicit-im2col dW tiles of the conv backward (TNS_OPT_DW_TILE = v) */
int         tns_conv_dw_tile_count(void);
/* plane-sized implicit-conv tiles (TNS_OPT_CONV_VARIANT = 100 + v) */
int         tns_conv_tile_variant_count(void);
const char* tns_conv_tile_variant_name(int32_t variant);
/* two-pass slab conv forms: the im2col matrix in the GEMM's LDS slot order,
 * then B by LDS-DMA (TNS_OPT_CONV_VARIANT = 500 + v) */
int         tns_conv_slab_count(void);
const char* tns_conv_slab_name(int32_t variant);
/* 1x1 stride-1 conv forms reading the input planes by LDS-DMA (planes of a
 * multiple of 4 pixels; TNS_OPT_CONV_VARIANT = 600 + v) */
int         tns_conv1x1_count(void);
const char* tns_conv1x1_name(int32_t variant);
/* VALU chain variants of the sdot-order NT product (TNS_OPT_SDOT_FORM = 1 + v) */
int         tns_sdot_chains_variant_count(void);
const char* tns_sdot_chains_variant_name(int32_t variant);
/* residue-register forms of the sdot-order NT product (TNS_OPT_SDOT_FORM =
 * 64 + v) */
int         tns_sdot_rc_variant_count(void);
const char* tns_sdot_rc_variant_name(int32_t variant);
const char* tns_gemm_variant_name(int32_t variant);
int tns_hip_gemm_variant(tns_ctx* ctx, int32_t variant, uint8_t transA, uint8_t transB,
                         int64_t M, int64_t N, int64_t K, float ALPHA,
                         const float* A, int64_t aOffset, int64_t lda, int64_t strideA,
                         const float* B, int64_t bOffset, int64_t ldb, int64_t strideB,
                         float BETA, float* C, int64_t cOffset, int64_t ldc, int64_t strideC,
                         int64_t batchCount);
/* Which kernel a GEMM would run on, without running it (no context, no device
 * call: the dispatch is a pure function of these numbers).  `variant` as
 * tns_hip_gemm_variant; `in` holds TNS_GP_COUNT values indexed by TNS_GP_*
 * (the shape as tns_hip_gemm_strided_batched takes it; ALPHA == 1 or not; the
 * beta mode: 0 C not read, 1 BETA == 1, 2 BETA * C; the epilogue: 0 none;
 * whether A and B are 16-byte aligned; the options TNS_OPT_NT_SDOT,
 * TNS_OPT_TT_EXACT and TNS_OPT_SDOT_FORM).  Writes one JSON object into `out`
 * (out_len bytes, 512 are enough): err (0, or TNS_ERR_UNSUPPORTED where the
 * forced variant refuses the problem, msg saying why), family (empty, tile,
 * nn_big, nt_sdot, sdot_chains, sdot_rc, tt), form and name within the family,
 * leaf (the kernel instantiation, one of tns_gemm_plan_leaf_name), and the
 * template choices: vec_a / vec_b (staging widths 4 or 1), rows / pre / alpha1
 * (large-NN forms 6..8), tn / vec / bk / o32 (the sdot-order MFMA kernel). */
enum { TNS_GP_TRANS_A = 0, TNS_GP_TRANS_B = 1, TNS_GP_M = 2, TNS_GP_N = 3, TNS_GP_K = 4,
       TNS_GP_LDA = 5, TNS_GP_LDB = 6, TNS_GP_LDC = 7, TNS_GP_STRIDE_A = 8, TNS_GP_STRIDE_B = 9,
       TNS_GP_STRIDE_C = 10, TNS_GP_BATCH = 11, TNS_GP_ALPHA_IS_ONE = 12, TNS_GP_BETA_MODE = 13,
       TNS_GP_EPI = 14, TNS_GP_A_ALIGNED16 = 15, TNS_GP_B_ALIGNED16 = 16, TNS_GP_NT_SDOT = 17,
       TNS_GP_TT_EXACT = 18, TNS_GP_SDOT_FORM = 19, TNS_GP_COUNT = 20 };
int         tns_gemm_plan(int32_t variant, const int64_t* in, char* out, int64_t out_len);
int         tns_gemm_plan_leaf_count(void);
const char* tns_gemm_plan_leaf_name(int32_t leaf);

/* TNS_OPT_STRICT_BETA0 (default 1): beta==0 computes 0*C like the reference
 * (NaN/Inf in C propagate).  0 = BLAS convention (C not read).
 * TNS_OPT_CONV_VARIANT (default -1 = heuristic): forces the tile shape of the
 * implicit-GEMM convolution (tuning; index as tns_gemm_variant_name, 100 + v
 * for plane-sized tile v of tns_conv_tile_variant_name, 500 + v for slab form
 * v of tns_conv_slab_name, 600 + v for 1x1 form v of tns_conv1x1_name;
 * 200..499 selected tile families that were removed: TNS_ERR_UNSUPPORTED).
 * TNS_OPT_CONV_PAD (default -1 = by cost): 1 gathers from a zero-padded copy
 * of the images, 0 bounds-checks the window inside the GEMM.
 * TNS_OPT_NT_SDOT (default 1): gemm(NoTrans, Trans) sums in the reference's
 * sdot_avx2 order (8 residue chains, ntensors.pas:1233-1306, 1957-2005), bit
 * for bit; 0 = one ascending-k chain per element (faster, within 1e-4).
 * TNS_OPT_SRSS_QUIRK (library default 0): 1 reproduces the reference's srss
 * dropping lanes 4..7 of the variance sum when a block is a multiple of 8
 * long (ntensors.pas:1493-1523, meansAndVars with blockSize % 8 == 0; and
 * sVarinceDelta_avx, 8739-8741).  The Pascal binding's initHIP and
 * useHipOpTable (pascal/nnHip.pas) set it to 1 by default, so a drop-in
 * reproduces the configured USE_AVX2 CPU build.
 * TNS_OPT_TT_EXACT (default 1): gemm(Trans, Trans) sums in the reference's
 * scalar s_tt order (mul, mul, add each rounded; ntensors.pas:2159-2182) on
 * the VALU, bit for bit; 0 = the fp32 MFMA kernel (faster, within 1e-4).
 * TNS_OPT_SDOT_FORM (default -1 = by shape): kernel of the sdot-order NT
 * product (tuning / tests; same result bit for bit): 0 = the MFMA kernel
 * (one wave per residue class), 1 + v = VALU chain kernel variant v (one
 * lane per few residue chains, for few outputs over a long k), 64 + v =
 * residue-register form v (one or two waves keep an output tile's eight
 * residue chains in their registers; many tiles over a short k).
 * TNS_OPT_DX_FUSED (default 1): the conv backward's state.delta of 1x1
 * stride-1, dilation-1 layers with >= 8192 pixels per image by one kernel that runs
 * each window tap's filter chain and adds it to the image pixel in scol2im's
 * order (no col matrix); 2 = that kernel on every stride-1 layer it fits;
 * 0 = the reference's two stages, TN GEMM into the workspace + col2im (same
 * bits in all three).
 * TNS_OPT_DX_TILE (default -1 = by shape): the first of those two stages,
 * col_b = W^T . delta_b, for all images in one launch of a k-major-A conv
 * tile (conv_tile4.hip, the delta planes as a 1x1 convolution's images) where
 * one applies; -2 = the TN GEMM always; v >= 0 forces form v of
 * tns_conv_dx_tile_count() (tests; same bits in every form).
 * TNS_OPT_DX_CONV (default -1 = by shape): the conv backward's state.delta of
 * stride-1, dilation-1 3x3 layers (C a multiple of 64, filters of 32) by one
 * implicit transposed convolution over the delta planes: each window tap's
 * filter chain, added to the image pixel in scol2im's (kr, kc) order for the
 * taps it does not skip — the TN GEMM + col2im sums, no col matrix (uses a
 * filters*C*9-float tap-major copy of the weights in the context's scratch);
 * -2 = off; v >= 0 forces form v of tns_conv_dx_conv_count() (same bits).
 * TNS_OPT_DW_TILE (default -1 = by shape): the conv backward's dW product
 * (the reference's per-image sdot-order NT GEMM over the im2col matrix) by
 * a kernel that generates the im2col rows in its staging (dw_tile.hip: no
 * col matrix, no im2col pass) where one applies; -2 = im2col + the sdot
 * kernels always; v >= 0 forces form v of tns_conv_dw_tile_count() (same
 * bits in every form).
 * TNS_OPT_DW_RES (default -1 = by shape): the conv backward's dW product as
 * the sdot order's eight residue chains run one after another per output
 * tile over residue-major copies of delta and the im2col matrix, folded in
 * sdot's order, then added to weight_updates image by image (dw_res.hip; the
 * copies and the per-group partial planes live in the context's scratch);
 * by shape on the 3x3 layers with >= 64 filters; -2 = off; v >= 0 forces
 * form v of tns_conv_dw_res_count() (same bits; ignored while
 * TNS_OPT_DW_TILE forces a tile).  Memory: the residue-major copies (about
 * the im2col matrix plus delta) and the group planes live in the context's
 * scratch, allocated IN ADDITION to the caller's workspace (which then holds
 * nothing for dW); -2 bounds the backward's dW memory to the workspace.
 * TNS_OPT_BWD_OVERLAP (default 1): the conv backward runs the dW product and
 * the state.delta chain (which read delta and write disjoint outputs)
 * concurrently, the latter on a side stream of the context that the
 * context's stream waits for before the call returns its work; 0 = in
 * sequence (also whenever telemetry is on).  Same results either way.
 * Memory: when dW reads an im2col matrix and state.delta takes the TN +
 * col2im chain, the overlap gives that chain its own batch*C*k*k*oH*oW-float
 * col buffer, allocated by the context IN ADDITION to the caller's workspace
 * (which then holds dW's col matrix only); if that allocation fails, or the
 * side stream cannot be created, the call runs in sequence within the
 * caller's workspace instead of failing.  Set 0 to bound the backward's
 * memory to the workspace.  2 = pipelined: each call enqueues its dW on the
 * side stream (behind the earlier calls' dW) and returns without joining it;
 * a later call whose operands meet a pending dW's (below), tns_hip_finish and
 * tns_hip_get_stream first make the context's stream wait for the side
 * stream.  The dW of layer L then runs under the following calls' derive /
 * state.delta work and the non-conv layers' calls between them; a later
 * backward call that writes into a pending dW's delta or input waits for that
 * dW first.  The caller must not read or modify a pending call's
 * weight_updates, nor modify its input or delta, by other means (work
 * enqueued on the stream outside this API, or host accesses) before a join:
 * tns_hip_finish, an entry point whose operands include them, or
 * tns_hip_get_stream (which joins before it hands the stream out, so work the
 * caller then enqueues on it is ordered after every pending dW).  Same results; state.delta always gets its own col buffer
 * (the memory note above).  pascal/nnHip.pas initHIP selects this mode by
 * default (pipelineBackward = true): there every access goes through the API.
 * Since round 6 no entry point joins unconditionally during a pipelined
 * pass: the non-conv ones (gemm, im2col / col2im, bias, activation, BLAS-1,
 * addvv & co, shortcut, upsample, yolo, pooling, batch norm, softmax, sgd_update)
 * join only when they write a pending dW's delta or input, read or write its
 * weight_updates (or the caller's workspace that dW's im2col fills), or take
 * a context scratch slot the side stream still uses — so TNet.backward's
 * shortcut / route / upsample calls between two conv layers keep the
 * pipeline running.  Context management, host copies, gemmBatched, the conv
 * forward drivers and the fused train step still join.
 * TNS_OPT_SCRATCH_CAP (default 0 = none): largest context scratch buffer in
 * floats; a larger request fails as a failed allocation does (tests reach the
 * fallback paths with it).
 * TNS_OPT_DERIVE_SUMS (default 0): 1 = the conv backward's Derivative and
 * addSums (no batch norm) in one pass where the sums' chain kernel applies
 * (planes under 16384 pixels); 0 = two passes (measured level: 15.06 vs
 * 15.00 ms a pipelined YOLOv3 pass, profiles/r04_bwd_schedules2.json).  Same
 * bits.
 * Environment switches read once per process (A/B timing only; every setting
 * gives the same bits): TNS_STREAM_PRIO=0 — the pipelined dW stream at the
 * default queue priority instead of the lowest (and the context's own stream
 * at the default instead of the highest); TNS_BN_FUSED=0 — batchNormBack as
 * its separate passes instead of the one chain pass + normalizeDelta;
 * TNS_DX_C1=0 — the 1x1 layers' state.delta on the TN product / conv_dx forms
 * instead of conv1x1's W^T product; TNS_ACC4=0 — the dW accumulate pass in
 * its scalar form. */
enum { TNS_OPT_STRICT_BETA0 = 0, TNS_OPT_CONV_VARIANT = 1, TNS_OPT_CONV_PAD = 2,
       TNS_OPT_NT_SDOT = 3, TNS_OPT_SRSS_QUIRK = 4, TNS_OPT_TT_EXACT = 5,
       TNS_OPT_SDOT_FORM = 6, TNS_OPT_DX_FUSED = 7, TNS_OPT_DX_TILE = 8,
       TNS_OPT_DW_TILE = 9, TNS_OPT_BWD_OVERLAP = 10, TNS_OPT_DX_CONV = 11,
       TNS_OPT_DW_RES = 12, TNS_OPT_DERIVE_SUMS = 13, TNS_OPT_SCRATCH_CAP = 14 };
int tns_set_option(int32_t opt, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* TNS_H */
