// tests/cpp/test_ordering.cpp -- the ordering of the reduced variables (gtsam_amd/csrc/ordering.cpp) on its own: no runtime, nothing
// preloaded.  Reverse Cuthill-McKee and minimum degree against naive versions on dense adjacency matrices written here, nested
// dissection by its properties, the two flop counts against a naive dense boolean Cholesky, the placement by hand-computed layouts.
// tests/test_ordering.py builds and runs it, plainly and under the address / undefined-behaviour sanitizers.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../gtsam_amd/csrc/ordering.h"

using namespace gt;

static int g_failed = 0, g_checked = 0;
static std::string g_case;
#define CHECK(cond) do { g_checked++; if (!(cond)) { if (g_failed++ < 40) std::printf("FAILED [%s] %s:%d: %s\n", g_case.c_str(), __FILE__, __LINE__, #cond); } } while (0)

typedef std::vector<int32_t> Ints;
typedef std::vector<std::vector<char>> Dense;

struct Edges {   // the off-diagonal blocks the way analysis.hip hands them over: pairs in any orientation
  int n = 0; Ints a, b;
  void add(int u, int v) { a.push_back(u); b.push_back(v); }
  BlockGraph graph() const { return BlockGraph(n, a, b); }
  Dense dense() const {
    Dense M(n, std::vector<char>(n, 0));
    for (size_t i = 0; i < a.size(); i++) if (a[i] != b[i]) M[a[i]][b[i]] = M[b[i]][a[i]] = 1;
    return M;
  }
};
static Edges path(int n) { Edges e; e.n = n; for (int i = 0; i + 1 < n; i++) e.add(i, i + 1); return e; }
static Edges cycle(int n) { Edges e = path(n); e.add(n - 1, 0); return e; }
static Edges star(int n) { Edges e; e.n = n; for (int i = 1; i < n; i++) e.add(i, 0); return e; }
static Edges grid(int rows, int cols) {
  Edges e; e.n = rows * cols;
  for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) {
    if (c + 1 < cols) e.add(r * cols + c, r * cols + c + 1);
    if (r + 1 < rows) e.add((r + 1) * cols + c, r * cols + c);
  }
  return e;
}
static Edges band(int n, int w) { Edges e; e.n = n; for (int i = 0; i < n; i++) for (int d = 1; d <= w && i + d < n; d++) e.add(i + d, i); return e; }
static Edges arrow(int n) { Edges e = path(n - 1); e.n = n; for (int i = 0; i + 1 < n; i++) e.add(n - 1, i); return e; }
static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static Edges random_sparse(int n, int m) {   // fixed seed; duplicates and a == b pairs on purpose
  Edges e; e.n = n; g_rng = 2024u;
  for (int i = 0; i < m; i++) e.add((int)(rnd() % n), (int)(rnd() % n));
  return e;
}
static Ints iota(int n) { Ints v(n); for (int i = 0; i < n; i++) v[i] = i; return v; }
static Ints shuffled(int n, uint32_t seed) {
  Ints v = iota(n); g_rng = seed;
  for (int i = n - 1; i > 0; i--) std::swap(v[i], v[rnd() % (i + 1)]);
  return v;
}
static bool is_permutation_of(Ints got, Ints want) { std::sort(got.begin(), got.end()); std::sort(want.begin(), want.end()); return got == want; }

// ---- reverse Cuthill-McKee, naively: level-synchronous searches on the dense matrix -----------------------------------------------
// visit order of a breadth-first search from s over the nodes still `in`, level by level, neighbours by ascending index
static Ints naive_bfs(const Dense& M, const std::vector<char>& in, int s, Ints& dist) {
  const int n = (int)M.size();
  dist.assign(n, -1); dist[s] = 0;
  Ints seen{s}, frontier{s};
  while (!frontier.empty()) {
    Ints next;
    for (int u : frontier) for (int w = 0; w < n; w++) if (M[u][w] && in[w] && dist[w] < 0) { dist[w] = dist[u] + 1; next.push_back(w); }
    seen.insert(seen.end(), next.begin(), next.end());
    frontier.swap(next);
  }
  return seen;
}
// of the farthest level the node of smallest degree; among equals the last one reached if it is one of them, else the first
static int naive_far(const Dense& M, const Ints& deg, const std::vector<char>& in, int s) {
  Ints dist; const Ints seen = naive_bfs(M, in, s, dist);
  const int far = dist[seen.back()];
  int lowest = deg[seen.back()];
  for (int v : seen) if (dist[v] == far) lowest = std::min(lowest, deg[v]);
  if (deg[seen.back()] == lowest) return seen.back();
  for (int v : seen) if (dist[v] == far && deg[v] == lowest) return v;
  return -1;
}
static Ints naive_rcm(const Dense& M, const Ints& nodes) {
  const int n = (int)M.size();
  Ints deg(n, 0);                                 // degree in the WHOLE graph, also for a subset
  for (int v = 0; v < n; v++) for (int w = 0; w < n; w++) deg[v] += M[v][w];
  std::vector<char> in(n, 0);
  for (int v : nodes) in[v] = 1;
  Ints visit;
  for (int seed : nodes) {
    if (!in[seed]) continue;
    const int start = naive_far(M, deg, in, naive_far(M, deg, in, seed));
    size_t head = visit.size();
    visit.push_back(start); in[start] = 0;
    for (; head < visit.size(); head++) {
      std::vector<std::pair<int, int>> nb;        // (degree, index)
      for (int w = 0; w < n; w++) if (M[visit[head]][w] && in[w]) { nb.push_back({deg[w], w}); in[w] = 0; }
      std::sort(nb.begin(), nb.end());
      for (auto& p : nb) visit.push_back(p.second);
    }
  }
  return Ints(visit.rbegin(), visit.rend());
}
static void check_rcm(const std::string& name, const Edges& e, const Ints& nodes) {
  g_case = "rcm " + name;
  const BlockGraph g = e.graph();
  const Ints got = rcm_order(g, nodes);
  CHECK(is_permutation_of(got, nodes));
  CHECK(got == naive_rcm(e.dense(), nodes));
}

// ---- nested dissection -----------------------------------------------------------------------------------------------------------
static void subtree_nodes(const std::vector<OrderingPart>& parts, int root, Ints& out) {
  out.insert(out.end(), parts[root].nodes.begin(), parts[root].nodes.end());
  for (int p = 0; p < (int)parts.size(); p++) if (parts[p].parent == root) subtree_nodes(parts, p, out);
}
static std::vector<OrderingPart> check_dissection(const std::string& name, const Edges& e, int depth, size_t want_parts) {
  g_case = "dissection " + name + " depth " + std::to_string(depth);
  const BlockGraph g = e.graph();
  const Dense M = e.dense();
  const std::vector<OrderingPart> parts = nested_dissection(g, depth);
  CHECK(parts.size() == want_parts);
  Ints all;
  int roots = 0;
  for (int p = 0; p < (int)parts.size(); p++) {
    all.insert(all.end(), parts[p].nodes.begin(), parts[p].nodes.end());
    CHECK(parts[p].parent == -1 || (parts[p].parent > p && parts[p].parent < (int)parts.size()));   // children are eliminated before their parent
    roots += parts[p].parent == -1;
    Ints set = parts[p].nodes; std::sort(set.begin(), set.end());
    CHECK(parts[p].nodes == rcm_order(g, set));
    Ints kids;
    for (int q = 0; q < (int)parts.size(); q++) if (parts[q].parent == p) kids.push_back(q);
    CHECK(kids.empty() || kids.size() == 2);
    if (kids.size() == 2) {                                     // a separator: no edge joins its two subtrees
      Ints A, B; subtree_nodes(parts, kids[0], A); subtree_nodes(parts, kids[1], B);
      bool joined = false;
      for (int u : A) for (int v : B) joined = joined || M[u][v];
      CHECK(!joined && !A.empty() && !B.empty());
    }
  }
  CHECK(roots == 1 && parts.back().parent == -1);
  CHECK(is_permutation_of(all, iota(e.n)));                     // every node in exactly one part
  const PartOrder po = flatten_parts(parts);
  CHECK(po.order == all);
  if (parts.size() == 1) CHECK(po.part_of_pos.empty() && po.part_parent.empty());
  else {
    CHECK(po.part_of_pos.size() == all.size() && po.part_parent.size() == parts.size());
    size_t at = 0;
    for (int p = 0; p < (int)parts.size(); p++) {
      CHECK(po.part_parent[p] == parts[p].parent);
      for (size_t k = 0; k < parts[p].nodes.size(); k++, at++) CHECK(po.part_of_pos[at] == p);
    }
  }
  return parts;
}

// ---- minimum degree, naively: the elimination graph as a dense matrix ----------------------------------------------------------------
static Ints naive_min_degree(Dense M) {
  const int n = (int)M.size();
  std::vector<char> gone(n, 0);
  Ints ord;
  for (int step = 0; step < n; step++) {
    int best = -1, best_deg = 0;
    for (int v = 0; v < n; v++) {
      if (gone[v]) continue;
      int d = 0;
      for (int w = 0; w < n; w++) d += M[v][w] && !gone[w];
      if (best < 0 || d < best_deg) { best = v; best_deg = d; }      // ascending v: ties go to the lowest index
    }
    ord.push_back(best); gone[best] = 1;
    for (int u = 0; u < n; u++) for (int w = 0; w < n; w++)
      if (u != w && !gone[u] && !gone[w] && M[best][u] && M[best][w]) M[u][w] = 1;
  }
  return ord;
}

// ---- the flop counts against a dense boolean Cholesky ----------------------------------------------------------------------------------
static void naive_fill(Dense& A) {   // symmetric boolean structure with its diagonal -> the same with fill
  const int n = (int)A.size();
  for (int k = 0; k < n; k++)
    for (int i = k + 1; i < n; i++) for (int j = k + 1; j < n; j++) if (A[i][k] && A[j][k]) A[i][j] = 1;
}
static double naive_block_flops(const Edges& e, const Ints& order, const Ints& dims) {
  const int n = e.n;
  Ints pos(n);
  for (int i = 0; i < n; i++) pos[order[i]] = i;
  Dense A(n, std::vector<char>(n, 0));
  for (int i = 0; i < n; i++) A[i][i] = 1;
  for (size_t i = 0; i < e.a.size(); i++) A[pos[e.a[i]]][pos[e.b[i]]] = A[pos[e.b[i]]][pos[e.a[i]]] = 1;
  naive_fill(A);
  double fl = 0.0;
  for (int j = 0; j < n; j++) {
    double s = 0.0;
    for (int i = j + 1; i < n; i++) if (A[i][j]) s += dims[order[i]];
    const double f = dims[order[j]];
    fl += f * f * f / 3.0 + f * f * s + f * s * s;
  }
  return fl;
}
static double naive_tile_flops(const Edges& e, const Ints& order, const Ints& dims, int tile) {
  const int n = e.n;
  Ints pos(n);
  std::vector<int64_t> first(n), last(n);             // first and last tile of the variable at every position
  int64_t o = 0;
  for (int i = 0; i < n; i++) { pos[order[i]] = i; first[i] = o / tile; o += dims[order[i]]; last[i] = (o - 1) / tile; }
  const int nt = (int)((o + tile - 1) / tile);
  Dense B(nt, std::vector<char>(nt, 0));
  auto mark = [&](int p, int q) { for (int64_t x = first[p]; x <= last[p]; x++) for (int64_t y = first[q]; y <= last[q]; y++) B[x][y] = B[y][x] = 1; };
  for (int i = 0; i < n; i++) mark(i, i);
  for (size_t i = 0; i < e.a.size(); i++) mark(pos[e.a[i]], pos[e.b[i]]);
  naive_fill(B);
  const double t3 = (double)tile * tile * tile;
  double fl = 0.0;
  for (int J = 0; J < nt; J++) {
    int left = 0;
    for (int k = 0; k < J; k++) left += B[J][k];
    fl += t3 / 3.0 + left * t3;                       // factor the diagonal tile, accumulate its updates
    for (int I = J + 1; I < nt; I++) {
      if (!B[I][J]) continue;
      int both = 0;
      for (int k = 0; k < J; k++) both += B[I][k] && B[J][k];
      fl += t3 + 2.0 * both * t3;                     // substitution, contraction steps
    }
  }
  return fl;
}
static bool close_rel(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::max(std::fabs(a), std::fabs(b)); }
static void check_flops(const std::string& name, const Edges& e, const Ints& dims, int want_tiles) {
  g_case = "flops " + name;
  const BlockGraph g = e.graph();
  int64_t total = 0;
  for (int d : dims) total += d;
  CHECK((total + 127) / 128 == want_tiles);
  const Ints orders[4] = {iota(e.n), rcm_order(g, iota(e.n)), min_degree_order(g), shuffled(e.n, 77u)};
  for (const Ints& order : orders) {
    CHECK(is_permutation_of(order, iota(e.n)));
    const double fb = block_level_flops(e.a, e.b, order, dims), ft = tile_level_flops(g, order, dims, 128);
    CHECK(fb > 0.0 && close_rel(fb, naive_block_flops(e, order, dims)));
    CHECK(ft > 0.0 && close_rel(ft, naive_tile_flops(e, order, dims, 128)));
  }
}

// ---- placement -------------------------------------------------------------------------------------------------------------------------
static std::vector<int64_t> range(int64_t a, int64_t b) { std::vector<int64_t> v; for (int64_t i = a; i < b; i++) v.push_back(i); return v; }
static std::vector<int64_t> concat(std::vector<int64_t> a, const std::vector<int64_t>& b) { a.insert(a.end(), b.begin(), b.end()); return a; }

int main() {
  // the adjacency lists: sorted, unique, a == b ignored
  {
    g_case = "block graph";
    Edges e; e.n = 4; e.add(2, 0); e.add(0, 2); e.add(1, 1); e.add(3, 0); e.add(0, 1); e.add(2, 0);
    const BlockGraph g = e.graph();
    CHECK(g.adj.size() == 4 && g.adj[0] == (Ints{1, 2, 3}) && g.adj[1] == (Ints{0}) && g.adj[2] == (Ints{0}) && g.adj[3] == (Ints{0}));
    CHECK(BlockGraph(3, Ints{}, Ints{}).adj == std::vector<Ints>(3));
  }

  check_rcm("path of 5", path(5), iota(5));
  check_rcm("cycle of 6", cycle(6), iota(6));
  check_rcm("star of 7", star(7), iota(7));                       // six leaves of degree 1: ties broken by index
  check_rcm("grid 4 x 4", grid(4, 4), iota(16));
  {
    Edges e = cycle(4); e.n = 9;                                  // a cycle, a path of 4 and the isolated node 8
    e.add(4, 5); e.add(6, 5); e.add(6, 7);
    check_rcm("two components and an isolated node", e, iota(9));
    check_rcm("the same, seeds in another order", e, Ints{8, 6, 7, 5, 4, 2, 0, 3, 1});
  }
  check_rcm("subset of a grid 4 x 4", grid(4, 4), Ints{0, 1, 2, 5, 6, 9, 10, 13, 15});   // 15 is cut off inside the subset
  check_rcm("subset of a star", star(7), Ints{2, 4, 6});          // the centre is outside: three components
  {
    g_case = "rcm path of 5, by hand";
    CHECK(rcm_order(path(5).graph(), iota(5)) == (Ints{0, 1, 2, 3, 4}) || rcm_order(path(5).graph(), iota(5)) == (Ints{4, 3, 2, 1, 0}));
  }

  // nested dissection: 256 nodes are dissected, 255 are one leaf
  for (int depth : {1, 2}) {
    const auto parts = check_dissection("grid 16 x 16", grid(16, 16), depth, 3);   // (the halves have fewer than 256 nodes: leaves at any depth)
    CHECK(parts[2].nodes.size() * 3 < 256 && std::min(parts[0].nodes.size(), parts[1].nodes.size()) * 20 >= 256 * 5);
    check_dissection("grid 15 x 17", grid(15, 17), depth, 1);
  }
  check_dissection("grid 16 x 16", grid(16, 16), 0, 1);
  {
    const auto parts = check_dissection("grid 32 x 32", grid(32, 32), 2, 7);       // two levels: both halves are dissected again
    CHECK(parts[2].parent == 6 && parts[5].parent == 6 && parts[0].parent == 2 && parts[1].parent == 2 && parts[3].parent == 5 && parts[4].parent == 5);
    check_dissection("grid 32 x 32", grid(32, 32), 1, 3);
  }
  {
    // layers of 1, 99, 100, 99, 1 nodes, consecutive layers fully connected: the only balanced level is the middle one, a third of the set
    Edges e; e.n = 300;
    const int first[6] = {0, 1, 100, 200, 299, 300};
    for (int l = 0; l < 4; l++)
      for (int u = first[l]; u < first[l + 1]; u++) for (int v = first[l + 1]; v < first[l + 2]; v++) e.add(u, v);
    check_dissection("layered cliques of 300", e, 2, 1);
    // ... and with one node fewer in the middle layer the separator is below a third: taken
    Edges f; f.n = 299;
    const int first2[6] = {0, 1, 100, 199, 298, 299};
    for (int l = 0; l < 4; l++)
      for (int u = first2[l]; u < first2[l + 1]; u++) for (int v = first2[l + 1]; v < first2[l + 2]; v++) f.add(u, v);
    const auto parts = check_dissection("layered cliques of 299", f, 1, 3);
    CHECK(parts[2].nodes.size() == 99);
  }
  {
    Edges e = path(256); e.n = 257;                               // a hub on a path: three BFS levels at most, no balanced one
    for (int i = 0; i < 256; i++) e.add(256, i);
    check_dissection("path of 256 with a hub", e, 2, 1);
  }
  {
    Edges e = path(128); e.n = 256;                               // two paths of 128: the second one is never reached and counts as "above"
    for (int i = 128; i + 1 < 256; i++) e.add(i, i + 1);
    const auto parts = check_dissection("two paths of 128", e, 1, 3);
    // levels of one node each; 8/20 below needs 103 nodes, the first such level is the separator
    CHECK(parts[0].nodes.size() == 103 && parts[1].nodes.size() == 152 && parts[2].nodes.size() == 1);
    Ints above = parts[1].nodes; std::sort(above.begin(), above.end());
    const Ints every = iota(256);
    CHECK(std::includes(above.begin(), above.end(), every.begin() + 128, every.end()));
  }

  // minimum degree
  for (const auto& named : {std::make_pair("path of 6", path(6)), std::make_pair("star of 7", star(7)), std::make_pair("grid 3 x 3", grid(3, 3)),
                            std::make_pair("random 20", random_sparse(20, 40))}) {
    g_case = std::string("minimum degree ") + named.first;
    const Ints got = min_degree_order(named.second.graph());
    CHECK(is_permutation_of(got, iota(named.second.n)));
    CHECK(got == naive_min_degree(named.second.dense()));
  }
  {
    g_case = "minimum degree star of 7, by hand";                 // leaves by index; the centre ties with the last leaf at degree 1 and has the lower index
    CHECK(min_degree_order(star(7).graph()) == (Ints{1, 2, 3, 4, 5, 0, 6}));
  }

  // flop counts: mixed dimensions 3 / 6 / 9, tile 128
  {
    Ints mixed(40);
    for (int i = 0; i < 40; i++) mixed[i] = 3 * (1 + (i * 7 + i / 3) % 3);
    int64_t total = 0;
    for (int d : mixed) total += d;
    const int tiles = (int)((total + 127) / 128);
    check_flops("band of 40", band(40, 3), mixed, tiles);
    check_flops("arrow of 40", arrow(40), mixed, tiles);
    check_flops("random sparse of 40", random_sparse(40, 90), mixed, tiles);
    Edges none; none.n = 40;
    check_flops("empty graph of 40", none, mixed, tiles);
    const Ints nines(60, 9);                                      // 540 columns: five tiles
    check_flops("band of 60, dimension 9", band(60, 4), nines, 5);
    check_flops("random sparse of 60, dimension 9", random_sparse(60, 150), nines, 5);
    check_flops("arrow of 60, dimension 9", arrow(60), nines, 5);
    Edges none60; none60.n = 60;
    check_flops("empty graph of 60, dimension 9", none60, nines, 5);
  }

  // placement
  {
    g_case = "placement, no parts";
    const Ints order{3, 0, 4, 1, 2}, dims{3, 6, 9, 6, 3};
    const Placement p = place_variables(order, Ints{}, dims, 128);
    CHECK(p.off == (std::vector<int64_t>{6, 12, 18, 0, 9}));        // positions: 3 at 0 (6 wide), 0 at 6 (3), 4 at 9 (3), 1 at 12 (6), 2 at 18 (9)
    CHECK(p.pad == range(27, 128) && p.NP == 128);
  }
  {
    g_case = "placement, no parts, a full tile";                  // nothing to pad
    const Placement p = place_variables(iota(32), Ints{}, Ints(32, 4), 128);
    CHECK(p.pad.empty() && p.NP == 128 && p.off[31] == 124);
  }
  {
    g_case = "placement, three parts";
    // 30, 10 and 5 variables of dimension 9: [0, 270) padded to 512, [512, 602) padded to 768, [768, 813) padded to 1024
    const int n = 45;
    Ints order(n), part(n), dims(n, 9);
    for (int i = 0; i < n; i++) { order[i] = n - 1 - i; part[i] = i < 30 ? 0 : i < 40 ? 1 : 2; }
    const Placement p = place_variables(order, part, dims, 128);
    for (int i = 0; i < n; i++) {
      const int64_t start = part[i] == 0 ? 0 : part[i] == 1 ? 512 : 768, before = part[i] == 0 ? 0 : part[i] == 1 ? 30 : 40;
      CHECK(p.off[order[i]] == start + 9 * (i - before));
      if (i == 0 || part[i] != part[i - 1]) CHECK(p.off[order[i]] % 256 == 0);
    }
    CHECK(p.pad == concat(concat(range(270, 512), range(602, 768)), range(813, 1024)) && p.NP == 1024);
  }
  {
    g_case = "placement, parts that end on the boundary";         // 256 columns + 128 columns: no pad between, the end aligned to 256
    Ints part(48, 0);
    for (int i = 32; i < 48; i++) part[i] = 1;
    const Placement p = place_variables(iota(48), part, Ints(48, 8), 128);
    CHECK(p.off[32] == 256 && p.pad == range(384, 512) && p.NP == 512);
  }
  {
    g_case = "placement, a single variable";
    const Placement p = place_variables(Ints{0}, Ints{}, Ints{6}, 128);
    CHECK(p.off == (std::vector<int64_t>{0}) && p.pad == range(6, 128) && p.NP == 128);
  }

  std::printf("%d checked, %d failed\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
