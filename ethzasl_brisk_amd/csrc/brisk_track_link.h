// The link rule of brisk_hip_link_tracks_device / brisk_hip_list_tracks_device: how the packed match lists of a chain of frames
// (what brisk_hip_select_pair_matches_device writes) become feature tracks.  `__host__ __device__`: the kernels of brisk_track.hip
// and the CPU test program tests/cpp/test_track_link.cc run the SAME code.  No function here is a CPU fallback of the product.
//
// A chain is `nodes` frames in time order; node i has n_i rows, of which the rows r < lim_i = min(max(n_i, 0), rows_cap) exist.
// Pair p has node p + 1 as query and node p as train; its records are matches[offsets[p] .. offsets[p + 1]).
//   Record j of pair p is a PROPOSAL iff it is the first record of its query row (j is the first of the range, or record j - 1 has
//   another queryIdx), 0 <= queryIdx < lim_{p+1}, 0 <= trainIdx < lim_p, and the bit pattern of its distance is <= 0x7F800000
//   (no NaN, no sign bit: for such floats the bit order is the numeric order).  Every other record is ignored.
//   Among the proposals for one train row the smallest key (distance bits << 32 | queryIdx) WINS: prev[p + 1][q] = t.  Every other
//   row has prev = -1; a loser does not fall back to its second entry.
//   A row with prev == -1 is a HEAD.  A head of node 0 with seed_track[r] >= 0 continues that track at seed_age[r]; every other
//   head STARTS a track at age 0, numbered first_new + the starting heads before it in (node, row) order.  An interior row has
//   its predecessor's track and its predecessor's age + 1.
//   A track piece (a head and the rows that follow it) is LISTED iff the age of its last row + 1 >= min_len.
// The 64-bit claim word of a train row holds the smallest key proposed for it: its low half is the winner's query row, so the
// word is the forward pointer of the chain as well.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BRISK_TRACK_HD __host__ __device__ inline
#else
#define BRISK_TRACK_HD inline
#endif

#define BRISK_TRACK_MAX_DISTANCE_BITS 0x7F800000u  // +INFINITY: the largest bit pattern that proposes
#define BRISK_TRACK_NO_CLAIM 0xFFFFFFFFFFFFFFFFull  // a train row nobody proposed for (no key reaches it: distance bits <= 0x7F800000)

// rows of a node that exist for the tracker
BRISK_TRACK_HD int brisk_track_lim(int n, int rows_cap) { return n < 0 ? 0 : (n < rows_cap ? n : rows_cap); }

// j: the record's index, begin: the first index of its pair's range, query_before: queryIdx of record j - 1 (read for j > begin only)
BRISK_TRACK_HD bool brisk_track_first_of_row(long long j, long long begin, int query, int query_before) {
  return j == begin || query_before != query;
}

BRISK_TRACK_HD bool brisk_track_proposes(bool first_of_row, int query, int train, unsigned distance_bits, int lim_query, int lim_train) {
  return first_of_row && query >= 0 && query < lim_query && train >= 0 && train < lim_train && distance_bits <= BRISK_TRACK_MAX_DISTANCE_BITS;
}

// (query >= 0 for a proposal)
BRISK_TRACK_HD unsigned long long brisk_track_key(unsigned distance_bits, int query) {
  return ((unsigned long long)distance_bits << 32) | (unsigned long long)(unsigned)query;
}

BRISK_TRACK_HD bool brisk_track_wins(unsigned long long claim, unsigned long long key) { return claim == key; }

// the row that follows train row t in the chain: the winner of its claim word, -1 = the track ends here
BRISK_TRACK_HD int brisk_track_next_row(unsigned long long claim) { return claim == BRISK_TRACK_NO_CLAIM ? -1 : (int)(unsigned)(claim & 0xFFFFFFFFull); }

BRISK_TRACK_HD bool brisk_track_is_head(int prev) { return prev < 0; }

// a head that gets a new number (seed_track: the seed of its row, read for node 0 with a seed only)
BRISK_TRACK_HD bool brisk_track_starts(int prev, int node, bool seeded, long long seed_track) {
  return brisk_track_is_head(prev) && !(node == 0 && seeded && seed_track >= 0);
}

BRISK_TRACK_HD bool brisk_track_listed(int last_age, int min_len) { return (long long)last_age + 1 >= (long long)min_len; }
