/* Micro-averaged ROC curve of the eval stage on the device: the curve that `aucroc+` keeps (reference src/evl/metric.py:36-41, sklearn's
 * roc_curve(Y.toarray().ravel(), Y_.toarray().ravel())), from the one streaming pass over the n * M scores that ntf_auc_micro_dense / ntf_auc_micro_csr make
 * (opentf_amd.h).  A header of its own beside opentf_amd.h (whose status codes and NTF_AUC_CHUNK_BYTES it uses): the two entries are handle-less, live in the
 * same libopentf_amd.so and do not change NTF_ABI_VERSION.
 *
 * The two entries mirror the AUC pair argument for argument (scores dense f32 [n, M] with ld floats per row, or CSR whose unstored entries score 0.0; the truth
 * CSR, rows, chunk_bytes as there) and add a caller-allocated curve.  Scores are compared as real numbers through the same monotone u32 key (auc_key): -0.0 ties
 * with +0.0, denormals are distinct, +-inf are ordinary values.
 *
 * Definitions.  v[0, G): the ascending distinct keys of the positives' scores.  pos_eq[g] / neg_eq[g]: the positives / negatives scoring exactly v[g].
 * Gap g (0 .. G): the scores strictly between v[g - 1] and v[g]; gap G lies above v[G - 1], gap 0 below v[0].  Only negatives lie in a gap.  c[g]: the number of
 * scores in gap g, m[g]: the smallest key among them.  value(): the inverse of the key; the key of either zero comes back as +0.0f.
 *
 * The points, in descending score order, with running integers fps = tps = 0:
 *   point 0 is (0, 0, +inf);
 *   for g = G down to 0:
 *     if c[g] > 0:  fps += c[g];                              emit (fps, tps, value(m[g]))
 *     if g >= 1:    fps += neg_eq[g - 1]; tps += pos_eq[g - 1]; emit (fps, tps, value(v[g - 1]))
 * There are at most 2 G + 2 <= 2 P + 2 points, and the last one is (N, P).  *n_points receives their number; fps / tps / thresholds [cap_points] receive them.
 * fpr = fps / N and tpr = tps / P are the caller's two divisions.
 *
 * What this list is.  It is the corner list of sklearn's micro-averaged ROC curve: the same piecewise-linear function, and every listed point, threshold included,
 * is a point of roc_curve(..., drop_intermediate=False) - between two consecutive positive scores the curve is one horizontal run, whose far end is the
 * smallest score of the gap.  It is NOT sklearn's drop_intermediate=True list (roc_curve's default), which also keeps points inside a gap wherever two
 * neighbouring negative-only scores have different multiplicities: that list needs the run length of every distinct score, i.e. a sort of the n * M pairs.  Every
 * point of either sklearn list lies on this polyline.
 *
 * out_counts = { P, N, U2 } and *out_auc = U2 / (2 P N): exactly what the AUC entries return for the same input.  U2 equals the curve's own doubled trapezoid,
 * sum over a of (fps[a + 1] - fps[a]) * (tps[a + 1] + tps[a]), as integers; the finish checks it.
 *
 * NTF_EINVAL, every output untouched: a null output pointer; cap_points < 2 P + 2 (P: the truth's stored entries over the selected rows, known to the caller
 * before the call); and every refusal of the AUC entries (opentf_amd.h: a null pointer or non-positive size, ld < M, a bad row / column index, a NaN score,
 * P == 0 or N == 0, 2 P N >= 2^64, a chunk budget below one row / one entry) - validated before any device call where those validate.
 * NTF_EHIP: no HIP device (there is no CPU fallback), or an integrity check of the finish failed (a gap's minimum outside its gap, a minimum in an empty gap,
 * a trapezoid that is not U2, or one of the AUC finish's own two checks). */
#ifndef OPENTF_AMD_ROC_H
#define OPENTF_AMD_ROC_H
#include "opentf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

int ntf_roc_micro_dense(int device, const float* scores, int64_t n, int64_t M, int64_t ld,
                        const int64_t* truth_indptr, const int32_t* truth_indices, int64_t n_truth_rows, const int64_t* rows,
                        int64_t chunk_bytes, int64_t cap_points,
                        uint64_t* fps /* [cap_points] */, uint64_t* tps /* [cap_points] */, float* thresholds /* [cap_points] */, int64_t* n_points,
                        uint64_t out_counts[3], double* out_auc);

int ntf_roc_micro_csr(int device, const int64_t* s_indptr, const int32_t* s_indices, const float* s_values, int64_t n, int64_t M,
                      const int64_t* truth_indptr, const int32_t* truth_indices, int64_t n_truth_rows, const int64_t* rows,
                      int64_t chunk_bytes, int64_t cap_points,
                      uint64_t* fps /* [cap_points] */, uint64_t* tps /* [cap_points] */, float* thresholds /* [cap_points] */, int64_t* n_points,
                      uint64_t out_counts[3], double* out_auc);

#ifdef __cplusplus
}
#endif
#endif /* OPENTF_AMD_ROC_H */
