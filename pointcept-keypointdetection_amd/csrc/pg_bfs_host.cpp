// Host side of PointGroup's clustering: the breadth-first search over directed neighbour lists that the reference runs
// in libs/pointgroup_ops/src/bfs_cluster.cpp:53-100 (find_cc / get_clusters) and the list layout of :102-111
// (fill_cluster_idxs_), restated from the algorithm.  Plain C++ with no dependency on the rest of the library, so a
// stand-alone program can link this file alone (tests/pg_bfs_host_main.cpp).
//
// The lists are DIRECTED: point j is in i's list when it is among the first `len` rows of start_len[i]; with lists cut
// at 1000 entries j's list need not hold i.  A component is what is reachable from its seed through same-label entries
// that no earlier component has taken; seeds are visited in ascending index, so a component's seed is its smallest
// member and components come out ordered by smallest member.  Members are written in discovery order.
#include <stddef.h>
#include <stdint.h>
#include <vector>

extern "C" int ptv3_pg_bfs_cluster_host(const int32_t* semantic_label, const int32_t* ball_query_idxs, int64_t n_active,
                                        const int32_t* start_len, int64_t n, int threshold, int32_t* cluster_idxs,
                                        int32_t* cluster_offsets, int32_t* counts) {
  if (n < 0 || n_active < 0 || n > INT32_MAX || !counts || !cluster_offsets) return 1;
  if (n > 0 && (!semantic_label || !start_len || !cluster_idxs)) return 1;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t start = start_len[2 * i], len = start_len[2 * i + 1];
    if (start < 0 || len < 0 || start + len > n_active) return 2;
  }
  for (int64_t e = 0; e < n_active; ++e)
    if (ball_query_idxs[e] < 0 || ball_query_idxs[e] >= n) return 2;

  std::vector<uint8_t> taken((size_t)n, 0);
  std::vector<int32_t> comp;  // members in discovery order; the part behind `head` is the queue
  int32_t n_cluster = 0;
  int64_t sum = 0;
  cluster_offsets[0] = 0;
  for (int64_t seed = 0; seed < n; ++seed) {
    if (taken[seed]) continue;
    comp.clear();
    comp.push_back((int32_t)seed);
    taken[seed] = 1;
    for (size_t head = 0; head < comp.size(); ++head) {
      const int32_t cur = comp[head];
      const int32_t label = semantic_label[cur];
      const int32_t* list = ball_query_idxs + start_len[2 * (int64_t)cur];
      const int32_t len = start_len[2 * (int64_t)cur + 1];
      for (int32_t e = 0; e < len; ++e) {
        const int32_t j = list[e];
        if (taken[j] || semantic_label[j] != label) continue;
        taken[j] = 1;
        comp.push_back(j);
      }
    }
    if ((int64_t)comp.size() < (int64_t)threshold) continue;
    for (size_t m = 0; m < comp.size(); ++m) {
      cluster_idxs[2 * (sum + (int64_t)m)] = n_cluster;
      cluster_idxs[2 * (sum + (int64_t)m) + 1] = comp[m];
    }
    sum += (int64_t)comp.size();
    cluster_offsets[++n_cluster] = (int32_t)sum;
  }
  counts[0] = n_cluster;
  counts[1] = (int32_t)sum;
  return 0;
}
