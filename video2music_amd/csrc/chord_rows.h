// What the kernels over (rows, 159) chord logits share (metrics.hip, chord_loss.hip): the vocabulary's constants, the emotion table
// of the reference's tgt_emotion rows, a row's three lane-strided dwords and the logits form of BCE.
#pragma once
#include "amt_common.h"

namespace {

constexpr int NC = 159, ID_END = 157, ID_PAD = 158;     // utilities/constants.py:50-52

// emotion class -> chord qualities it accepts (dataset/vevo_dataset.py:461-475), bit q-1 for quality q = 1..13 in the order
// maj dim sus4 min7 min sus2 aug dim7 maj6 hdim7 7 min6 maj7
constexpr uint32_t qrow(const char (&s)[14]) {
    uint32_t m = 0;
    for (int i = 0; i < 13; ++i) m |= (s[i] == '1' ? 1u : 0u) << i;
    return m;
}
constexpr uint32_t Q_EXCITING = qrow("1010000000100"), Q_FEARFUL = qrow("0101000101000"), Q_TENSE = qrow("0111000000100"),
                   Q_SAD = qrow("0001110000000"), Q_RELAXING = qrow("1000000010001");
__device__ __forceinline__ uint32_t quality_mask(int emo) {
    return emo == 0 ? Q_EXCITING : emo == 1 ? Q_FEARFUL : emo == 2 ? Q_TENSE : emo == 3 ? Q_SAD : emo == 4 ? Q_RELAXING : 0u;
}

__device__ __forceinline__ void load_row(const float* __restrict__ p, int lane, float& y0, float& y1, float& y2) {
    y0 = p[lane];
    y1 = p[lane + 64];
    y2 = lane < NC - 128 ? p[lane + 128] : -INFINITY;
}

// max(y,0) - y*t + log1p(exp(-|y|)): torch's binary_cross_entropy_with_logits
__device__ __forceinline__ float bce_term(float y, bool t) {
    return (fmaxf(y, 0.0f) - (t ? y : 0.0f)) + log1pf(expf(-fabsf(y)));
}

}  // namespace
