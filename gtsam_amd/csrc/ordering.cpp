// ordering.cpp -- the fill-reducing order of the reduced variables (ordering.h): host code without a runtime underneath.
//
// The reference gets its elimination order from COLAMD (inference/Ordering.cpp:42-124) unless the user passes one; here the order
// only decides where each camera / pose block sits in S.  A banded / loop-closing block pattern then leaves most 128 x 128 tiles of
// the factor empty, and the tile schedule skips them.
#include "ordering.h"

#include <algorithm>
#include <iterator>
#include <set>
#include <utility>

namespace gt {

BlockGraph::BlockGraph(int n, const std::vector<int32_t>& a, const std::vector<int32_t>& b) : adj(n) {
  for (size_t i = 0; i < a.size(); i++)
    if (a[i] != b[i]) { adj[a[i]].push_back(b[i]); adj[b[i]].push_back(a[i]); }
  for (auto& l : adj) { std::sort(l.begin(), l.end()); l.erase(std::unique(l.begin(), l.end()), l.end()); }
}

namespace {

struct Search {   // breadth-first searches over the nodes marked active, and what is built on them
  const std::vector<std::vector<int32_t>>& adj;
  std::vector<int32_t> level;
  std::vector<char> active;     // node belongs to the subgraph being processed and is not ordered yet
  std::vector<OrderingPart> parts;
  explicit Search(const BlockGraph& g) : adj(g.adj), level(g.adj.size(), -1), active(g.adj.size(), 0) {}

  void bfs_levels(int start, std::vector<int32_t>& q) {   // BFS over active nodes, fills level[], q = the visit order
    q.assign(1, start);
    std::fill(level.begin(), level.end(), -1);
    level[start] = 0;
    for (size_t h = 0; h < q.size(); h++)
      for (int32_t w : adj[q[h]]) if (active[w] && level[w] < 0) { level[w] = level[q[h]] + 1; q.push_back(w); }
  }
  int far_node(int start) {   // of the last level, the node of smallest degree (first reached among equals)
    std::vector<int32_t> q; bfs_levels(start, q);
    int best = q.back();
    for (int32_t v : q) if (level[v] == level[q.back()] && adj[v].size() < adj[best].size()) best = v;
    return best;
  }
  void rcm(const std::vector<int32_t>& nodes, std::vector<int32_t>& out) {
    for (int32_t v : nodes) active[v] = 1;
    out.reserve(nodes.size());
    for (int32_t seed : nodes) {
      if (!active[seed]) continue;
      const int start = far_node(far_node(seed));   // two sweeps towards a pseudo-peripheral node of the component
      std::vector<int32_t> q{start}; active[start] = 0;
      for (size_t h = 0; h < q.size(); h++) {
        std::vector<int32_t> nb;
        for (int32_t w : adj[q[h]]) if (active[w]) { active[w] = 0; nb.push_back(w); }
        std::sort(nb.begin(), nb.end(), [&](int32_t a, int32_t b) { return adj[a].size() < adj[b].size() || (adj[a].size() == adj[b].size() && a < b); });
        q.insert(q.end(), nb.begin(), nb.end());
      }
      out.insert(out.end(), q.begin(), q.end());
    }
    std::reverse(out.begin(), out.end());
  }
  // The elimination tree gets independent subtrees, i.e. the tile Cholesky gets several serial chains that run side by side instead
  // of one.  Returns the index of the part that roots this subtree (its last part in elimination order).
  int dissect(const std::vector<int32_t>& nodes, int depth) {
    if (depth > 0 && nodes.size() >= 256) {
      for (int32_t v : nodes) active[v] = 1;
      std::vector<int32_t> q;
      bfs_levels(far_node(far_node(nodes[0])), q);
      const int L = level[q.back()];
      std::vector<int64_t> cnt(L + 2, 0), pre(L + 2, 0);
      for (int32_t v : q) cnt[level[v]]++;
      for (int l = 0; l <= L; l++) pre[l + 1] = pre[l] + cnt[l];
      const int64_t n = (int64_t)nodes.size();
      int best = -1;
      // balance first (the parts become chains of diagonal tiles that run side by side: the longest one is the critical path), then
      // the smallest separator among the balanced cuts; a cut that leaves a quarter on each side is the fallback
      for (int64_t share : {10, 8, 5})
        if (best < 0)
          for (int l = 1; l < L; l++) {
            const int64_t below = pre[l], above = n - pre[l + 1];   // nodes not reached by the BFS count as "above"
            if (std::min(below, above) * 20 < n * share) continue;
            if (best < 0 || cnt[l] < cnt[best]) best = l;
          }
      for (int32_t v : nodes) active[v] = 0;
      if (best > 0 && cnt[best] * 3 < n) {
        std::vector<int32_t> A, B, S;
        for (int32_t v : nodes) (level[v] >= 0 && level[v] < best ? A : level[v] == best ? S : B).push_back(v);
        const int ra = dissect(A, depth - 1), rb = dissect(B, depth - 1);
        parts.emplace_back();
        const int me = (int)parts.size() - 1;
        rcm(S, parts[me].nodes);
        parts[ra].parent = parts[rb].parent = me;
        return me;
      }
    }
    parts.emplace_back();
    rcm(nodes, parts.back().nodes);
    return (int)parts.size() - 1;
  }
};

}  // namespace

std::vector<int32_t> rcm_order(const BlockGraph& g, const std::vector<int32_t>& nodes) {
  Search s(g);
  std::vector<int32_t> out;
  s.rcm(nodes, out);
  return out;
}

std::vector<OrderingPart> nested_dissection(const BlockGraph& g, int depth) {
  Search s(g);
  std::vector<int32_t> all(g.adj.size());
  for (size_t i = 0; i < all.size(); i++) all[i] = (int32_t)i;
  s.dissect(all, depth);
  return std::move(s.parts);
}

PartOrder flatten_parts(const std::vector<OrderingPart>& parts) {
  PartOrder o;
  for (size_t pi = 0; pi < parts.size(); pi++) {
    o.order.insert(o.order.end(), parts[pi].nodes.begin(), parts[pi].nodes.end());
    if (parts.size() == 1) break;
    o.part_of_pos.insert(o.part_of_pos.end(), parts[pi].nodes.size(), (int32_t)pi);
    o.part_parent.push_back(parts[pi].parent);
  }
  return o;
}

std::vector<int32_t> min_degree_order(const BlockGraph& g) {
  const int n = (int)g.adj.size();
  std::vector<std::set<int32_t>> e(n);
  for (int v = 0; v < n; v++) e[v].insert(g.adj[v].begin(), g.adj[v].end());
  std::set<std::pair<int32_t, int32_t>> heap;
  for (int v = 0; v < n; v++) heap.emplace((int32_t)e[v].size(), v);
  std::vector<int32_t> ord; ord.reserve(n);
  while (!heap.empty()) {
    const int v = heap.begin()->second; heap.erase(heap.begin());
    ord.push_back(v);
    const std::vector<int32_t> nb(e[v].begin(), e[v].end());
    for (int32_t w : nb) { heap.erase({(int32_t)e[w].size(), w}); e[w].erase(v); }
    for (int32_t w : nb) for (int32_t u : nb) if (u != w) e[w].insert(u);
    for (int32_t w : nb) heap.emplace((int32_t)e[w].size(), w);
    std::set<int32_t>().swap(e[v]);
  }
  return ord;
}

double block_level_flops(const std::vector<int32_t>& a, const std::vector<int32_t>& b, const std::vector<int32_t>& order, const std::vector<int32_t>& dims) {
  const int n = (int)order.size();
  std::vector<int32_t> pos(n);
  for (int i = 0; i < n; i++) pos[order[i]] = i;
  std::vector<std::vector<int32_t>> below(n), children(n);   // below: positions > own position
  for (size_t i = 0; i < a.size(); i++) {
    if (a[i] == b[i]) continue;
    const int pa = pos[a[i]], pb = pos[b[i]];
    below[std::min(pa, pb)].push_back(std::max(pa, pb));
  }
  std::vector<int32_t> merged;
  double fl = 0.0;
  for (int j = 0; j < n; j++) {
    std::vector<int32_t>& sj = below[j];
    std::sort(sj.begin(), sj.end()); sj.erase(std::unique(sj.begin(), sj.end()), sj.end());
    for (int32_t ch : children[j]) {                   // struct(j) |= struct(child) \ {j}
      merged.clear();
      std::set_union(sj.begin(), sj.end(), below[ch].begin(), below[ch].end(), std::back_inserter(merged));
      merged.erase(std::remove(merged.begin(), merged.end(), (int32_t)j), merged.end());
      sj.swap(merged);
      std::vector<int32_t>().swap(below[ch]);
    }
    double sdim = 0.0;
    for (int32_t q : sj) sdim += dims[order[q]];
    const double f = dims[order[j]];
    fl += f * f * f / 3.0 + f * f * sdim + f * sdim * sdim;
    if (!sj.empty()) children[sj.front()].push_back(j);
  }
  return fl;
}

// What the kernels execute is decided at TILE granularity: whole 128 x 128 tiles, fill included.  "auto" therefore scores the
// orderings by the flops over the tiles they would store (the count of tile_plan.cpp::plan_dataflow), not by the block-level count:
// on the street-network shape (datasets.py::synthetic_bal_streets, random long-range loop closures) minimum degree needs FEWER flops
// at block level (42 against 57 GFLOP) and 12 x MORE at tile level (1 170 against 101: its fill is scattered, 96 % of the tiles are
// touched) -- the first version of "auto" compared block-level counts and picked it.
double tile_level_flops(const BlockGraph& g, const std::vector<int32_t>& order, const std::vector<int32_t>& dims, int tile) {
  const int n = (int)order.size();
  std::vector<int64_t> off(n + 1, 0);
  std::vector<int32_t> pos(n);
  for (int i = 0; i < n; i++) { pos[order[i]] = i; off[i + 1] = off[i] + dims[order[i]]; }
  const int ntl = (int)((off[n] + tile - 1) / tile);
  std::vector<uint8_t> Bt((size_t)ntl * ntl, 0);
  auto mark = [&](int pa, int pb) {
    for (int64_t a = off[pa] / tile; a <= (off[pa + 1] - 1) / tile; a++)
      for (int64_t b = off[pb] / tile; b <= (off[pb + 1] - 1) / tile; b++) Bt[(size_t)std::max(a, b) * ntl + std::min(a, b)] = 1;
  };
  for (int v = 0; v < n; v++) { mark(pos[v], pos[v]); for (int32_t w : g.adj[v]) if (pos[w] < pos[v]) mark(pos[v], pos[w]); }
  for (int k = 0; k < ntl; k++) {
    std::vector<int> r;
    for (int i = k + 1; i < ntl; i++) if (Bt[(size_t)i * ntl + k]) r.push_back(i);
    for (size_t a = 0; a < r.size(); a++) for (size_t b = 0; b <= a; b++) Bt[(size_t)r[a] * ntl + r[b]] = 1;
  }
  const double t3 = (double)tile * tile * tile;
  double fl = 0.0;
  std::vector<int> cnt(ntl, 0);
  for (int i = 0; i < ntl; i++) for (int k = 0; k < i; k++) cnt[i] += Bt[(size_t)i * ntl + k];
  for (int J = 0; J < ntl; J++) {
    fl += t3 / 3.0 + cnt[J] * t3;
    for (int I = J + 1; I < ntl; I++) {
      if (!Bt[(size_t)I * ntl + J]) continue;
      int both = 0;
      for (int k = 0; k < J; k++) both += Bt[(size_t)I * ntl + k] & Bt[(size_t)J * ntl + k];
      fl += t3 + 2.0 * both * t3;
    }
  }
  return fl;
}

Placement place_variables(const std::vector<int32_t>& order, const std::vector<int32_t>& part_of_pos, const std::vector<int32_t>& dims, int tile) {
  Placement p;
  p.off.assign(order.size(), 0);
  int64_t o = 0;
  for (size_t pp = 0; pp < order.size(); pp++) {
    if (!part_of_pos.empty() && (pp == 0 || part_of_pos[pp] != part_of_pos[pp - 1]))
      while (o % (2 * tile)) p.pad.push_back(o++);
    p.off[order[pp]] = o; o += dims[order[pp]];
  }
  const int64_t align = part_of_pos.empty() ? tile : 2 * tile;
  while (o % align) p.pad.push_back(o++);
  p.NP = o;
  return p;
}

}  // namespace gt
