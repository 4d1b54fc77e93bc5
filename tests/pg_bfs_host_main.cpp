// Stand-alone check of ptv3_pg_bfs_cluster_host (csrc/pg_bfs_host.cpp) for a host sanitizer build: links that one source,
// touches no GPU.  Two inputs: a hand-built directed list set whose directed and undirected components differ, and a
// 3000-point pseudo-random graph, each compared with a queue-based search written here.  Exit status 0 = equal.
#include <stdint.h>
#include <stdio.h>
#include <deque>
#include <vector>

extern "C" int ptv3_pg_bfs_cluster_host(const int32_t* semantic_label, const int32_t* ball_query_idxs, int64_t n_active,
                                        const int32_t* start_len, int64_t n, int threshold, int32_t* cluster_idxs,
                                        int32_t* cluster_offsets, int32_t* counts);

static int check(const std::vector<int32_t>& label, const std::vector<std::vector<int32_t>>& lists, int threshold) {
  const int64_t n = (int64_t)label.size();
  std::vector<int32_t> idx, start_len;
  for (const auto& l : lists) {
    start_len.push_back((int32_t)idx.size());
    start_len.push_back((int32_t)l.size());
    idx.insert(idx.end(), l.begin(), l.end());
  }
  std::vector<int32_t> got_idxs(2 * n), got_offs(n + 1);
  int32_t counts[2] = {-1, -1};
  if (ptv3_pg_bfs_cluster_host(label.data(), idx.data(), (int64_t)idx.size(), start_len.data(), n, threshold,
                               got_idxs.data(), got_offs.data(), counts) != 0) return 1;
  std::vector<int32_t> want_idxs, want_offs(1, 0);
  std::vector<char> seen(n, 0);
  for (int32_t s = 0; s < n; ++s) {
    if (seen[s]) continue;
    std::vector<int32_t> comp(1, s);
    std::deque<int32_t> q(1, s);
    seen[s] = 1;
    while (!q.empty()) {
      const int32_t cur = q.front();
      q.pop_front();
      for (int32_t j : lists[cur])
        if (!seen[j] && label[j] == label[cur]) { seen[j] = 1; comp.push_back(j); q.push_back(j); }
    }
    if ((int)comp.size() < threshold) continue;
    for (int32_t m : comp) { want_idxs.push_back((int32_t)want_offs.size() - 1); want_idxs.push_back(m); }
    want_offs.push_back(want_offs.back() + (int32_t)comp.size());
  }
  if (counts[0] != (int32_t)want_offs.size() - 1 || counts[1] != want_offs.back()) return 2;
  for (size_t i = 0; i < want_offs.size(); ++i) if (got_offs[i] != want_offs[i]) return 3;
  for (size_t i = 0; i < want_idxs.size(); ++i) if (got_idxs[i] != want_idxs[i]) return 4;
  return 0;
}

int main() {
  // 0 -> 1 -> 2, 3 -> 2 (3 reaches 2 but nothing reaches 3), 4 alone with a foreign-label entry
  std::vector<int32_t> label = {7, 7, 7, 7, 9};
  std::vector<std::vector<int32_t>> lists = {{0, 1}, {1, 2}, {2}, {3, 2}, {4, 0}};
  int rc = check(label, lists, 1);
  if (rc) { printf("hand-built case failed: %d\n", rc); return 10 + rc; }
  const int n = 3000;
  uint32_t x = 12345u;
  auto next = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
  label.assign(n, 0);
  lists.assign(n, {});
  for (int i = 0; i < n; ++i) {
    label[i] = (int32_t)(next() % 3);
    const int deg = (int)(next() % 4);
    lists[i].push_back(i);
    for (int d = 0; d < deg; ++d) lists[i].push_back((int32_t)(next() % n));
  }
  for (int threshold : {1, 5}) {
    rc = check(label, lists, threshold);
    if (rc) { printf("random graph failed at threshold %d: %d\n", threshold, rc); return 20 + rc; }
  }
  // an entry outside the arrays is refused, not followed
  int32_t bad_label[1] = {0}, bad_idx[1] = {5}, bad_sl[2] = {0, 1}, out_idxs[2], out_offs[2], counts[2];
  if (ptv3_pg_bfs_cluster_host(bad_label, bad_idx, 1, bad_sl, 1, 1, out_idxs, out_offs, counts) != 2) return 30;
  printf("pg_bfs_host ok\n");
  return 0;
}
