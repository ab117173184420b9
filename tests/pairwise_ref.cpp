// pairwise_ref.cpp — the end score of one sequence against another under two-piece affine gaps, in int64: the plain pairwise DP that the
// exhaustive reference of the general POA path (tests/exhlib.py) runs once per source-to-sink path of a graph. It knows no graph, no
// predecessor lists and no sinks: a path is a string. Three ends: global (both sequences whole), local (any cell, at least 0) and overlap
// (free ends on both sequences: a start in row 0 or column 0, an end in the last row or the last column). M ends in a pair, X1 / X2 in a
// letter of a against a gap under the first / the second piece, Y1 / Y2 in a letter of b against a gap. A linear gap is the caller's
// e = q = c = g, an affine one (q, c) = (g, e). tests/test_poa_exhaustive_ref.py pins it to the recurrences in Python integers of
// tests/test_poa_convex_ref.py (gotoh2). The tests compile this file with g++ and load it through ctypes.
//
//   pw_score(a, n, b, L, mode, sc)              mode 0 local, 1 global, 2 overlap; sc: the six scores m, x, g, e, q, c. n, L >= 1
//   pw_max(text, off, n_paths, b, L, mode, sc)  the maximum of pw_score over the strings text[off[k] .. off[k + 1]); n_paths >= 1
#include <algorithm>
#include <cstdint>
#include <vector>

namespace {

constexpr int64_t NEG = INT64_MIN / 4;
enum { SW = 0, NW = 1, OV = 2 };

int64_t end_score(const char* a, int64_t n, const char* b, int64_t L, int mode, const int64_t* sc) {
    const int64_t m = sc[0], x = sc[1], g = sc[2], e = sc[3], q = sc[4], c = sc[5];
    // one row in place: T the cell maximum, X1 / X2 the gaps that come down the column
    std::vector<int64_t> T(L + 1, 0), X1(L + 1, NEG), X2(L + 1, NEG);
    if (mode == NW) for (int64_t j = 1; j <= L; j++) T[j] = std::max(g + (j - 1) * e, q + (j - 1) * c);
    int64_t best = mode == SW ? 0 : NEG;
    for (int64_t i = 1; i <= n; i++) {
        int64_t diag = T[0];
        if (mode == NW) { X1[0] = g + (i - 1) * e; X2[0] = q + (i - 1) * c; T[0] = std::max(X1[0], X2[0]); }
        int64_t y1 = NEG, y2 = NEG;
        for (int64_t j = 1; j <= L; j++) {
            const int64_t up = T[j];
            int64_t pair = diag + (a[i - 1] == b[j - 1] ? m : x);
            if (mode == SW) pair = std::max<int64_t>(pair, 0);
            const int64_t x1 = std::max(up + g, X1[j] + e), x2 = std::max(up + q, X2[j] + c);
            y1 = std::max(T[j - 1] + g, y1 + e);
            y2 = std::max(T[j - 1] + q, y2 + c);
            const int64_t h = std::max(std::max(pair, std::max(x1, x2)), std::max(y1, y2));
            diag = up; T[j] = h; X1[j] = x1; X2[j] = x2;
            if (mode == SW || (mode == OV && (i == n || j == L))) best = std::max(best, h);
        }
    }
    return mode == NW ? T[L] : best;
}

}  // namespace

extern "C" int64_t pw_score(const char* a, int64_t n, const char* b, int64_t L, int32_t mode, const int64_t* sc) { return end_score(a, n, b, L, mode, sc); }

extern "C" int64_t pw_max(const char* text, const int64_t* off, int64_t n_paths, const char* b, int64_t L, int32_t mode, const int64_t* sc) {
    int64_t best = INT64_MIN;
    for (int64_t k = 0; k < n_paths; k++) best = std::max(best, end_score(text + off[k], off[k + 1] - off[k], b, L, mode, sc));
    return best;
}
