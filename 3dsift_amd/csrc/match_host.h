// match_host.h -- the O(n) host bookkeeping of muBruteMatcher::bijectMatchBase (reference Src/cMatcher.cc:81-144), replayed exactly
// as written there, sign-flip quirks included (an index 0 that is "rejected" stays 0).  Shared by sift3d_match (kernels_match.hip) and
// sift3d_match_guided (entry_match_guided.hip), which differ only in the columns a row's best and second best are taken over.
#pragma once
#include <stddef.h>

#include <vector>

namespace s3d {

// filter, Src/cMatcher.cc:81-97
inline void match_ratio_filter(std::vector<int> &gi, const std::vector<float> &gd, const std::vector<float> &sd, double thresHold) {
	const double t2 = thresHold * thresHold;
	for (size_t i = 0; i < gi.size(); i++) {
		if (gi[i] < 0) continue;
		if ((double)(gd[i] / sd[i]) >= t2) gi[i] *= -1;
	}
}

// countMatched :114-120 and toMask :122-131 over a filtered forward result: cnt[j] = 1 where target j is masked in (mode 2: matched at
// least once, mode 3: more than once); returns the masked targets in ascending order -- the rows of the reverse pass
inline std::vector<int> match_mask_rows(const std::vector<int> &gi, int m, int mode, std::vector<int> &cnt) {
	const int mask_thres = (mode == 2) ? 0 : 1;
	cnt.assign(m, 0);
	for (size_t i = 0; i < gi.size(); i++)
		if (gi[i] >= 0) cnt[gi[i]] += 1;
	std::vector<int> rows;
	for (int j = 0; j < m; j++) {
		cnt[j] = cnt[j] > mask_thres ? 1 : 0;
		if (cnt[j]) rows.push_back(j);
	}
	return rows;
}

// bijectFilter :133-144; gi2: the filtered reverse result (masked-out targets hold -1)
inline void match_biject(std::vector<int> &gi, const std::vector<int> &cnt, const std::vector<int> &gi2) {
	for (size_t i = 0; i < gi.size(); i++) {
		const int j = gi[i];
		if (j < 0 || cnt[j] == 0) continue;
		if (gi2[j] != (int)i) gi[i] *= -1;
	}
}

// toCvec :99-112: the rows (ref rx, ry, rz, tar rx, ry, rz) of the surviving pairs in ascending ref index into pairs6 (may be NULL);
// returns their number
inline int match_to_cvec(const std::vector<int> &gi, const float *rx, const float *tx, float *pairs6) {
	int np = 0;
	for (size_t i = 0; i < gi.size(); i++) {
		const int j = gi[i];
		if (j < 0) continue;
		if (pairs6)
			for (int c = 0; c < 3; c++) {
				pairs6[(size_t)np * 6 + c] = rx[i * 3 + c];
				pairs6[(size_t)np * 6 + 3 + c] = tx[(size_t)j * 3 + c];
			}
		np++;
	}
	return np;
}

}  // namespace s3d
