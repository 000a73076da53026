// pair_truncate.h -- the "longest_first" truncation of a (first, second) text pair, one copy for the host tokenizer (wordpiece.hip) and the
// device pair assembly (rerank.hip).
#pragma once
#include <hip/hip_runtime.h>

// Lengths (n1, n2) the two sides keep of (len1, len2) tokens under `budget` = max_len - 3, as the `tokenizers` library computes them
// (AutoTokenizer's default fast backend): nothing is cut when both fit; only the longer side is cut when that suffices; otherwise both go to
// budget / 2 and the odd token goes to the longer side (to the second on equal lengths).
__host__ __device__ inline void rmu_longest_first(int len1, int len2, int budget, int* keep1, int* keep2) {
    int n1 = len1, n2 = len2;
    if (n1 + n2 > budget) {
        const bool swap = n1 > n2;
        if (swap) { const int t = n1; n1 = n2; n2 = t; }
        n2 = n1 > budget ? n1 : (n1 > budget - n1 ? n1 : budget - n1);
        if (n1 + n2 > budget) { n1 = budget / 2; n2 = n1 + budget % 2; }
        if (swap) { const int t = n1; n1 = n2; n2 = t; }
    }
    *keep1 = n1 < len1 ? n1 : len1;
    *keep2 = n2 < len2 ? n2 : len2;
}
