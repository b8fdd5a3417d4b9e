// tests/cpp/test_tile_plan.cpp -- the tile schedules' planner (gtsam_amd/csrc/tile_plan.cpp) on its own: no runtime, nothing preloaded.
// Structure only, no numerics: fill against a naive boolean Cholesky, the stored list and its slot table, the dataflow task list
// (contraction lists, pieces, ticket order, chains) and the tables resolved to slots.  tests/test_tile_plan.py builds and runs it,
// plainly and under the address / undefined-behaviour sanitizers.
#include <algorithm>
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../gtsam_amd/csrc/tile_plan.h"

using namespace gt;

static int g_failed = 0, g_checked = 0;
static std::string g_case;
#define CHECK(cond) do { g_checked++; if (!(cond)) { if (g_failed++ < 40) std::printf("FAILED [%s] %s:%d: %s\n", g_case.c_str(), __FILE__, __LINE__, #cond); } } while (0)

typedef std::vector<uint8_t> Bytes;
typedef std::vector<int32_t> Ints;

// the lower triangle after a boolean Cholesky written out naively: (i, j) becomes non-zero when both (i, k) and (j, k) are
static Bytes naive_fill(int n, const Bytes* s) {
  std::vector<std::vector<char>> A(n, std::vector<char>(n, 0));
  for (int i = 0; i < n; i++) for (int j = 0; j <= i; j++) A[i][j] = A[j][i] = (i == j || !s || (*s)[(size_t)i * n + j]) ? 1 : 0;
  for (int k = 0; k < n; k++)
    for (int i = k + 1; i < n; i++) for (int j = k + 1; j < n; j++) if (A[i][k] && A[j][k]) A[i][j] = 1;
  Bytes L((size_t)n * n, 0);
  for (int i = 0; i < n; i++) for (int j = 0; j <= i; j++) L[(size_t)i * n + j] = A[i][j];
  return L;
}

template <class F> static Bytes lower(int n, F pred) {
  Bytes s((size_t)n * n, 0);
  for (int i = 0; i < n; i++) for (int j = 0; j <= i; j++) s[(size_t)i * n + j] = pred(i, j) ? 1 : 0;
  return s;
}
// what analysis.hip hands the stream schedule: a column pair holds something where one of its tiles does
static Bytes pairs_of(int nt, const Bytes& s) {
  const int np = (nt + 1) / 2;
  Bytes p((size_t)np * np, 0);
  for (int i = 0; i < nt; i++) for (int j = 0; j <= i; j++) if (s[(size_t)i * nt + j]) p[(size_t)(i / 2) * np + j / 2] = 1;
  return p;
}

struct Case {
  std::string name; int nt;
  const Bytes* tiles;                        // nullptr = dense
  const Ints* pair_part; const Ints* part_parent;
};

static void check_stream_schedule(const Case& c, const Bytes& tile_fill, CholLists& cl) {
  const int nt = c.nt, np = (nt + 1) / 2;
  Bytes ps; if (c.tiles) ps = pairs_of(nt, *c.tiles);
  const Bytes pair_fill = symbolic_fill(np, c.tiles ? &ps : nullptr);
  CHECK(pair_fill == naive_fill(np, c.tiles ? &ps : nullptr));
  const CholTables t = plan_chol(cl, nt, c.tiles ? &ps : nullptr, c.pair_part, c.part_parent);
  CHECK(cl.h_fill == pair_fill && cl.nt == nt && !cl.stream_lists);
  // the stored list: no duplicate, every filled tile (of either granularity) and the rhs row; h_slot is its inverse
  std::set<std::pair<int, int>> stored;
  CHECK((int64_t)t.stored.size() == 2 * cl.n_stored && cl.h_slot.size() == (size_t)(nt + 1) * nt);
  for (int64_t q = 0; q < cl.n_stored; q++) {
    const int I = t.stored[2 * q], J = t.stored[2 * q + 1];
    CHECK(I >= J && I <= nt && J >= 0 && J < nt);
    CHECK(stored.insert({I, J}).second);
    CHECK(cl.h_slot[(size_t)I * nt + J] == q);
  }
  CHECK((int64_t)std::count_if(cl.h_slot.begin(), cl.h_slot.end(), [](int32_t q) { return q >= 0; }) == cl.n_stored);
  for (int I = 0; I < nt; I++) for (int J = 0; J <= I; J++) {
    if (pair_fill[(size_t)(I / 2) * np + J / 2]) CHECK(stored.count({I, J}) == 1);
    if (tile_fill[(size_t)I * nt + J]) CHECK(stored.count({I, J}) == 1);
  }
  for (int J = 0; J < nt; J++) CHECK(stored.count({nt, J}) == 1);
  // TRSM rows and the backward lists name stored tiles only; the backward tiles by column are the ones by row
  for (int k = 0; k < nt; k++) for (int64_t e = cl.trsm_off[k]; e < cl.trsm_off[k] + cl.trsm_cnt[k]; e++) CHECK(stored.count({t.rows[e], k}) == 1);
  std::set<std::pair<int, int>> by_row, by_col;
  for (int kt = 0; kt < nt; kt++) for (int64_t e = cl.bwd_off[kt]; e < cl.bwd_off[kt] + cl.bwd_cnt[kt]; e++) { CHECK(stored.count({kt, t.bcols[e]}) == 1); by_row.insert({kt, t.bcols[e]}); }
  CHECK((int)t.bwd_col_off.size() == nt + 1);
  for (int jt = 0; jt < nt; jt++) for (int e = t.bwd_col_off[jt]; e < t.bwd_col_off[jt + 1]; e++) {
    by_col.insert({t.bwd_col_rows[e], jt});
    if (e > t.bwd_col_off[jt]) CHECK(t.bwd_col_rows[e] < t.bwd_col_rows[e - 1]);   // rows descending
  }
  CHECK(by_row == by_col);
  // the pair lists: every update (I, J) of a column pair hits stored tiles; with parts some cross into the separator
  const Ints pairs = plan_stream_pairs(cl);
  int64_t listed = 0, crossing = 0;
  for (int p = 0; p < np; p++) {
    const int64_t off[4] = {cl.s1_off[p], cl.nar_off[p], cl.rest_off[p], cl.anc_off[p]}, cnt[4] = {cl.s1_cnt[p], cl.nar_cnt[p], cl.rest_cnt[p], cl.anc_cnt[p]};
    for (int l = 0; l < 4; l++) {
      listed += cnt[l]; if (l == 3) crossing += cnt[l];
      for (int64_t e = off[l]; e < off[l] + cnt[l]; e++) {
        const int I = pairs[2 * e], J = pairs[2 * e + 1];
        CHECK(stored.count({I, J}) == 1 && stored.count({I, 2 * p}) == 1 && stored.count({J, 2 * p}) == 1);
        if (l == 3) CHECK((*c.pair_part)[J / 2] != (*c.pair_part)[p]);
      }
    }
  }
  CHECK(listed == (int64_t)pairs.size() / 2 || (listed == 0 && pairs.size() == 2));
  CHECK((crossing > 0) == (c.pair_part != nullptr));
  CHECK(cl.critical_pairs == (c.pair_part ? 3 : np));   // (the parts of this file: two pairs of the longer leaf + the separator)
}

struct TilePieces { std::vector<int64_t> ticket; std::vector<PieceRec> rec; };

static void check_dataflow_schedule(const Case& c, const CholLists& cl) {
  const int nt = c.nt;
  Ints tile_part;
  if (c.pair_part) for (int tl = 0; tl < nt; tl++) tile_part.push_back((*c.pair_part)[tl / 2]);
  const TileFill fill = df_fill_rows(nt, c.tiles);
  const ColumnOrder order = df_column_sequence(nt, c.pair_part ? &tile_part : nullptr, c.part_parent);
  DfLists df;
  plan_dataflow(df, nt, c.tiles, c.pair_part ? &tile_part : nullptr, c.part_parent);
  const Ints& pos = order.pos;
  auto filled = [&](int I, int k) { return I == nt || fill.B[(size_t)I * nt + k] != 0; };
  // seq: a permutation, pos its inverse; interleaved when there are parts
  CHECK(df.h_seq == order.seq && (int)df.h_seq.size() == nt && df.nt == nt);
  { Ints s = df.h_seq; std::sort(s.begin(), s.end()); for (int q = 0; q < nt; q++) { CHECK(s[q] == q); CHECK(pos[df.h_seq[q]] == q); } }
  if (c.pair_part) CHECK(order.tree && tile_part[df.h_seq[0]] != tile_part[df.h_seq[1]]);
  else for (int q = 0; q < nt; q++) CHECK(df.h_seq[q] == q);
  // chains: the lists partition the block columns, every workgroup walks its tiles in pos order
  CHECK(df.n_chain == (int)df.h_chain_off.size() - 1 && df.h_chain_off.front() == 0 && df.h_chain_off.back() == nt && (int)df.h_chain_tiles.size() == nt);
  CHECK(df.n_chain == (c.pair_part ? 4 : nt > 1 ? 2 : 1));
  { Ints s = df.h_chain_tiles; std::sort(s.begin(), s.end()); for (int q = 0; q < nt; q++) CHECK(s[q] == q); }
  for (int w = 0; w < df.n_chain; w++) {
    CHECK(df.h_chain_off[w] <= df.h_chain_off[w + 1]);
    for (int e = df.h_chain_off[w] + 1; e < df.h_chain_off[w + 1]; e++) CHECK(pos[df.h_chain_tiles[e - 1]] < pos[df.h_chain_tiles[e]]);
  }
  // tasks by tile
  CHECK((int64_t)df.h_tasks.size() == 6 * df.n_tasks);
  std::map<std::pair<int, int>, TilePieces> tiles;
  for (int64_t tk = 0; tk < df.n_tasks; tk++) {
    const int32_t* d = df.h_tasks.data() + 6 * tk;
    CHECK(d[0] >= d[1] && d[0] <= nt && d[1] >= 0 && d[1] < nt);
    CHECK(cl.h_slot[(size_t)d[0] * nt + d[1]] >= 0);                     // every tile of the task list has a slot
    TilePieces& tp = tiles[{d[0], d[1]}];
    tp.ticket.push_back(tk); tp.rec.push_back(PieceRec{d[0], d[1], d[2], d[3], d[4], d[5]});
  }
  size_t expected_tiles = 0;
  for (int J = 0; J < nt; J++) for (int I = J; I <= nt; I++) if (filled(I, J)) { expected_tiles++; CHECK(tiles.count({I, J}) == 1); }
  CHECK(tiles.size() == expected_tiles);
  std::map<std::pair<int, int>, int64_t> final_ticket;
  for (const auto& kv : tiles) final_ticket[kv.first] = kv.second.ticket.back();
  int max_pieces = 1;
  for (const auto& kv : tiles) {
    const int I = kv.first.first, J = kv.first.second;
    const TilePieces& tp = kv.second;
    // the contraction list: {k < J : fill(I, k) and fill(J, k)} by pos; a diagonal tile with has_sub leaves column J - 1 to the chain kernel
    if (I == J) CHECK((df.h_has_sub[J] != 0) == (J > 0 && filled(J, J - 1)));
    Ints want;
    for (int k = 0; k < J; k++) if (filled(I, k) && filled(J, k) && !(I == J && k == J - 1 && df.h_has_sub[J])) want.push_back(k);
    std::stable_sort(want.begin(), want.end(), [&](int a, int b) { return pos[a] < pos[b]; });
    // pieces 0 .. R - 1 once each, tickets increasing, ranges adjacent and covering the list
    const int R = tp.rec[0].R;
    max_pieces = std::max(max_pieces, R);
    CHECK(R >= 1 && R < (int)kPieceBase && (int)tp.rec.size() == R);
    int64_t at = tp.rec[0].koff, total = 0;
    for (size_t r = 0; r < tp.rec.size(); r++) {
      const PieceRec& p = tp.rec[r];
      CHECK(p.r == (int)r && p.R == R && p.koff == at && p.kcnt >= 0);
      if (r + 1 < tp.rec.size()) CHECK(p.kcnt > 0);
      if (r > 0) CHECK(tp.ticket[r] > tp.ticket[r - 1]);
      at += p.kcnt; total += p.kcnt;
    }
    CHECK(total == (int64_t)want.size() && at <= (int64_t)df.h_klist.size());
    if (total == (int64_t)want.size()) for (size_t e = 0; e < want.size(); e++) CHECK(df.h_klist[tp.rec[0].koff + e] == want[e]);
    // an early piece is queued behind the block column of its youngest operand: behind every last piece of that column, and so
    // behind the last pieces of all the tiles it reads
    for (size_t r = 0; r + 1 < tp.rec.size(); r++) {
      const PieceRec& p = tp.rec[r];
      int young = df.h_klist[p.koff];
      for (int e = p.koff; e < p.koff + p.kcnt; e++) {
        const int k = df.h_klist[e];
        if (pos[k] > pos[young]) young = k;
        if (I < nt) CHECK(final_ticket.at({I, k}) < tp.ticket[r]);
        CHECK(final_ticket.at({J, k}) < tp.ticket[r]);
      }
      for (const auto& other : tiles) if (other.first.second == young) CHECK(other.second.ticket.back() < tp.ticket[r]);
      CHECK(pos[young] < pos[J] - 1);   // (two groups before the tile's own column at the latest)
    }
  }
  // resolved tables
  DfLists df2 = df;
  const Ints lane_tab = df_lane_table(df2, cl.h_slot, cl.n_stored);
  const DfTables tab = df_resolve_host(df2, cl.h_slot, nullptr, lane_tab);
  const Ints chain = df_chain_words(df2, cl.h_slot, nullptr);
  auto slot = [&](int I, int J) { return cl.h_slot[(size_t)I * nt + J]; };
  CHECK(tab.tasks.size() == (size_t)kTaskWords * df.n_tasks && tab.steps.size() == (size_t)kStepWords * df.h_klist.size() && tab.skipped == 0.0);
  CHECK(lane_tab.size() == 2 * (size_t)cl.n_stored);
  std::vector<char> scratch_used((size_t)df2.n_scratch, 0);
  int64_t lanes_total = 0, tiles_with_lanes = 0;
  for (int64_t q = 0; q < cl.n_stored; q++) {
    const int G = lane_tab[2 * q], first = lane_tab[2 * q + 1];
    if (G == 1) { CHECK(first == -1); continue; }
    CHECK(G >= 2 && G <= 8 && first >= cl.n_stored && first + (G - 1) <= cl.n_stored + df2.n_scratch);
    for (int64_t s = first; s < first + G - 1 && s < cl.n_stored + df2.n_scratch; s++) { CHECK(!scratch_used[s - cl.n_stored]); scratch_used[s - cl.n_stored] = 1; }
    lanes_total += G - 1; tiles_with_lanes++;
  }
  CHECK(lanes_total == df2.n_scratch);
  for (const auto& kv : tiles) {   // a tile gets lanes from 8 early pieces on
    const int E = kv.second.rec[0].R - 1;
    CHECK((lane_tab[2 * (size_t)slot(kv.first.first, kv.first.second)] > 1) == (E >= 8));
  }
  for (int64_t tk = 0; tk < df.n_tasks; tk++) {
    const int32_t* d = df.h_tasks.data() + 6 * tk; const int32_t* o = tab.tasks.data() + kTaskWords * tk;
    for (int x = 0; x < 6; x++) CHECK(o[x] == d[x]);
    CHECK(o[6] == slot(d[0], d[1]) && o[7] == slot(d[1], d[1]));
    CHECK(o[8] == lane_tab[2 * (size_t)o[6]] && o[9] == lane_tab[2 * (size_t)o[6] + 1]);
    for (int e = d[2]; e < d[2] + d[3]; e++) {
      const int32_t* w = tab.steps.data() + kStepWords * (size_t)e;
      CHECK(w[0] == slot(d[0], df.h_klist[e]) && w[1] == slot(d[1], df.h_klist[e]));
    }
  }
  CHECK(chain.size() == (size_t)kChainWords * nt);
  for (int J = 0; J < nt; J++) { CHECK(chain[kChainWords * J] == slot(J, J)); CHECK(chain[kChainWords * J + 1] == (df.h_has_sub[J] ? slot(J, J - 1) : -1)); }
  if (c.name == "dense40") CHECK(max_pieces > 8 && tiles_with_lanes > 0 && df2.n_scratch > 0);   // early pieces and accumulator lanes are reached
  else CHECK(df2.n_scratch == 0);
  std::printf("%-10s nt %2d: %lld tasks, %d chain workgroups, up to %d pieces, %lld scratch slots\n", c.name.c_str(), nt, (long long)df.n_tasks, df.n_chain, max_pieces, (long long)df2.n_scratch);
}

int main() {
  const Bytes banded = lower(9, [](int i, int j) { return i - j <= 2; });
  const Bytes arrow = lower(7, [](int i, int j) { return i == j || i == 6; });
  const Bytes arrow_rev = lower(7, [](int i, int j) { return i == j || j == 0; });   // (the arrow the other way round: fills the whole triangle)
  // column pairs {0, 1} and {2} are leaves that do not touch, pair {3} is their separator
  const Ints pair_part = {0, 0, 1, 2}, part_parent = {2, 2, -1};
  const Bytes parts = lower(8, [&](int i, int j) { return pair_part[i / 2] == pair_part[j / 2] || pair_part[i / 2] == 2; });
  const std::vector<Case> cases = {
    {"dense1", 1, nullptr, nullptr, nullptr}, {"dense2", 2, nullptr, nullptr, nullptr}, {"dense3", 3, nullptr, nullptr, nullptr},
    {"dense5", 5, nullptr, nullptr, nullptr}, {"banded9", 9, &banded, nullptr, nullptr}, {"arrow7", 7, &arrow, nullptr, nullptr},
    {"arrow7rev", 7, &arrow_rev, nullptr, nullptr},
    {"parts8", 8, &parts, &pair_part, &part_parent}, {"dense40", 40, nullptr, nullptr, nullptr},
  };
  for (const Case& c : cases) {
    g_case = c.name;
    const Bytes tile_fill = symbolic_fill(c.nt, c.tiles);
    CHECK(tile_fill == naive_fill(c.nt, c.tiles));
    if (c.name == "banded9") CHECK(tile_fill == banded);                      // no fill
    if (c.name == "arrow7") CHECK(tile_fill == arrow);                        // (this way round the arrow leaves the tiles as they are;
    if (c.name == "arrow7rev") CHECK(tile_fill == lower(7, [](int, int) { return true; }) && tile_fill != arrow_rev);   // this way it fills them all)
    CholLists cl;
    check_stream_schedule(c, tile_fill, cl);
    check_dataflow_schedule(c, cl);
  }
  std::printf("%d checks, %d failed\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
