// A word's confidence in 2^-19 fixed point: the fp32 max-subtracted softmax mass that its logit row gives to a set of classes.
// One definition for the region confidences (regions.hip: the set is "the classes of the word's kind") and the block confidences
// (block_scores.hip: the set is a bit mask per category, and one word is scored against several masks from ONE set of
// exponentials).  Both forms take the same terms in the same (ascending class) order into `num` and `den`, so for the same set
// they give the same bits: num <= den, and q == 2^19 exactly where every class is in the set.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// q = p * 2^19 rounded: a page has <= 4096 = 2^12 words and p <= 1, so a sum of q over a page is <= 2^31 -- an unsigned 32-bit word
constexpr float GTE_SCORE_ONE = 524288.0f;
constexpr int GTE_SCORE_PAGE_MAX = 4096;
static_assert((uint64_t)GTE_SCORE_PAGE_MAX * (uint64_t)GTE_SCORE_ONE <= 0xFFFFFFFFull, "the fixed-point sum must fit 32 bits");

__device__ __forceinline__ unsigned gte_score_quantise(float num, float den) {       // den >= exp(0) = 1
    return (unsigned)((num / den) * GTE_SCORE_ONE + 0.5f);
}

// p(v) in 2^-19 fixed point: the mass of row `lg` on the classes c with class_group[c] == kind; 0 for a row with a non-finite
// logit.  Any number of classes: the exponentials are formed in the loop that adds them.
__device__ __forceinline__ unsigned region_word_score(const float* __restrict__ lg, int n_classes,
                                                      const int32_t* __restrict__ class_group, int kind) {
    float m = lg[0];
    bool finite = isfinite(m);
    for (int c = 1; c < n_classes; ++c) {
        const float x = lg[c];
        finite = finite && isfinite(x);
        m = fmaxf(m, x);
    }
    if (!finite) return 0u;
    float den = 0.f, num = 0.f;
    for (int c = 0; c < n_classes; ++c) {
        const float e = expf(lg[c] - m);
        den += e;
        if (class_group[c] == kind) num += e;
    }
    return gte_score_quantise(num, den);
}

// The same for <= 16 classes with the exponentials kept: load() once per word, score(mask) once per set.  Every index of e[] is
// a constant of an unrolled loop, so the array lives in registers.
constexpr int GTE_SCORE_MAX_CLASSES = 16;
struct WordExps {
    float e[GTE_SCORE_MAX_CLASSES];
    float den;
    bool finite;

    __device__ __forceinline__ void load(const float* __restrict__ lg, int n_classes) {
        float x[GTE_SCORE_MAX_CLASSES];
        float m = lg[0];
        x[0] = m;
        finite = isfinite(m);
#pragma unroll
        for (int c = 1; c < GTE_SCORE_MAX_CLASSES; ++c) {
            x[c] = c < n_classes ? lg[c] : m;
            finite = finite && isfinite(x[c]);
            m = fmaxf(m, x[c]);
        }
        den = 0.f;
#pragma unroll
        for (int c = 0; c < GTE_SCORE_MAX_CLASSES; ++c) {
            e[c] = c < n_classes ? expf(x[c] - m) : 0.f;
            if (c < n_classes) den += e[c];
        }
    }
    // mask: bit c set = class c is in the set (bits at and above n_classes must be clear)
    __device__ __forceinline__ unsigned score(unsigned mask) const {
        if (!finite) return 0u;
        float num = 0.f;
#pragma unroll
        for (int c = 0; c < GTE_SCORE_MAX_CLASSES; ++c)
            if ((mask >> c) & 1u) num += e[c];
        return gte_score_quantise(num, den);
    }
};
