// tile_plan.cpp -- the tile schedules of the reduced-system Cholesky (tile_plan.h): host code without a runtime underneath.
#include "tile_plan.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <utility>

namespace gt {

namespace {
constexpr double kTile3 = (double)kTile * kTile * kTile;   // flops / 2 of one tile-by-tile product
}

std::vector<uint8_t> symbolic_fill(int n, const std::vector<uint8_t>* structure) {
  std::vector<uint8_t> B((size_t)n * n, 0);
  for (int i = 0; i < n; i++)
    for (int j = 0; j <= i; j++) B[(size_t)i * n + j] = structure ? (*structure)[(size_t)i * n + j] : 1;
  for (int i = 0; i < n; i++) B[(size_t)i * n + i] = 1;
  std::vector<int> r;
  for (int k = 0; k < n; k++) {   // symbolic elimination: the rows of column k become a clique
    r.clear();
    for (int i = k + 1; i < n; i++) if (B[(size_t)i * n + k]) r.push_back(i);
    for (size_t a = 0; a < r.size(); a++)
      for (size_t b = 0; b <= a; b++) B[(size_t)r[a] * n + r[b]] = 1;
  }
  return B;
}

// ---- stream schedule ---------------------------------------------------------------------------------------------------------------
namespace {

// the row tiles below column pair p, pair p's own excluded
void rows_below_pair(const std::vector<uint8_t>& B, int np, int nt, int p, std::vector<int32_t>& R) {
  R.clear();
  for (int q = p + 1; q < np; q++) if (B[(size_t)q * np + p]) tiles_of(q, nt, R);
}

// TRSM row lists, the stored list and the flops, column pair by column pair; returns the stored lower tiles
int64_t chol_forward_lists(CholLists& plan, const std::vector<uint8_t>& B, CholTables& t) {
  const int nt = plan.nt, np = (nt + 1) / 2;
  double flops = 0.0; int64_t stored = 0;
  std::vector<int32_t> R;
  for (int p = 0; p < np; p++) {
    const int k = 2 * p; const bool two = k + 1 < nt;
    rows_below_pair(B, np, nt, p, R);
    stored += (two ? 3 : 1) + (int64_t)R.size() * (two ? 2 : 1);
    for (int cc = k; cc <= (two ? k + 1 : k); cc++) {
      for (int rr = cc; rr <= (two ? k + 1 : k); rr++) { t.stored.push_back(rr); t.stored.push_back(cc); }
      for (int32_t I : R) { t.stored.push_back(I); t.stored.push_back(cc); }
      t.stored.push_back(nt); t.stored.push_back(cc);
    }
    // column k: rows below = [k+1] + R + [rhs]
    plan.trsm_off[k] = (int64_t)t.rows.size();
    if (two) t.rows.push_back(k + 1);
    t.rows.insert(t.rows.end(), R.begin(), R.end()); t.rows.push_back(nt);
    plan.trsm_cnt[k] = (int64_t)t.rows.size() - plan.trsm_off[k];
    flops += kTile3 / 3.0 + (double)(plan.trsm_cnt[k] - 1) * kTile3;
    if (two) {
      flops += (double)((int64_t)R.size() + 1) * 2.0 * kTile3;     // (the thin update's pairs: (k + 1, k + 1), (I, k + 1) for I in R; the rhs row's excluded)
      plan.trsm_off[k + 1] = (int64_t)t.rows.size();
      t.rows.insert(t.rows.end(), R.begin(), R.end()); t.rows.push_back(nt);
      plan.trsm_cnt[k + 1] = (int64_t)t.rows.size() - plan.trsm_off[k + 1];
      flops += kTile3 / 3.0 + (double)(plan.trsm_cnt[k + 1] - 1) * kTile3;
    }
    const double kk = two ? 2.0 : 1.0;
    flops += (double)((int64_t)R.size() * ((int64_t)R.size() + 1) / 2) * 2.0 * kTile3 * kk;   // rhs row excluded
  }
  plan.flops = flops;
  return stored;
}

// backward solve: the non-zero column tiles of every row tile, and the same tiles by column, rows descending (what the one-launch
// backward sweep walks)
void chol_backward_lists(CholLists& plan, const std::vector<uint8_t>& B, CholTables& t) {
  const int nt = plan.nt, np = (nt + 1) / 2;
  for (int kt = 0; kt < nt; kt++) {
    plan.bwd_off[kt] = (int64_t)t.bcols.size();
    const int q = kt / 2;
    for (int p = 0; p < q; p++) if (B[(size_t)q * np + p]) tiles_of(p, nt, t.bcols);
    if (kt & 1) t.bcols.push_back(kt - 1);
    plan.bwd_cnt[kt] = (int64_t)t.bcols.size() - plan.bwd_off[kt];
  }
  std::vector<std::vector<int32_t>> by_col(nt);
  for (int kt = nt - 1; kt >= 0; kt--)
    for (int64_t e = plan.bwd_off[kt]; e < plan.bwd_off[kt] + plan.bwd_cnt[kt]; e++) by_col[t.bcols[e]].push_back(kt);
  t.bwd_col_off.assign(nt + 1, 0);
  for (int jt = 0; jt < nt; jt++) { t.bwd_col_rows.insert(t.bwd_col_rows.end(), by_col[jt].begin(), by_col[jt].end()); t.bwd_col_off[jt + 1] = (int32_t)t.bwd_col_rows.size(); }
}

// pairs on the longest leaf-to-root path of the parts
int chol_critical_pairs(const CholLists& plan, int np) {
  if (plan.pair_part.empty()) return np;
  const int nparts = (int)plan.part_parent.size();
  std::vector<int> len(nparts, 0), path(nparts, 0);
  for (int p = 0; p < np; p++) len[plan.pair_part[p]]++;
  int best = 0;
  for (int x = nparts - 1; x >= 0; x--) {   // parents have larger indices: walk down from the root
    const int par = plan.part_parent[x];
    path[x] = len[x] + (par >= 0 ? path[par] : 0);
    best = std::max(best, path[x]);
  }
  return best;
}

}  // namespace

// Symbolic factorisation at the granularity of 256-wide column pairs (the unit the trailing update contracts
// over), then the per-pair tile lists.  This is the reduced system's elimination structure: what the reference
// rebuilds as EliminationTree + JunctionTree on every lambda try (inference/EliminationTree-inst.h:77-155,
// JunctionTree-inst.h:63-151), computed once here.
CholTables plan_chol(CholLists& plan, int nt, const std::vector<uint8_t>* pair_struct,
                     const std::vector<int32_t>* pair_part, const std::vector<int32_t>* part_parent) {
  const int np = (nt + 1) / 2;
  plan.pair_part.clear(); plan.part_parent.clear();
  if (pair_part && !pair_part->empty()) { plan.pair_part = *pair_part; plan.part_parent = *part_parent; }
  plan.nt = nt;
  plan.trsm_off.assign(nt, 0); plan.trsm_cnt.assign(nt, 0);
  plan.s1_off.assign(np, 0); plan.s1_cnt.assign(np, 0); plan.nar_off.assign(np, 0); plan.nar_cnt.assign(np, 0);
  plan.rest_off.assign(np, 0); plan.rest_cnt.assign(np, 0); plan.anc_off.assign(np, 0); plan.anc_cnt.assign(np, 0);
  plan.bwd_off.assign(nt, 0); plan.bwd_cnt.assign(nt, 0);
  // (the SYRK pair lists of the stream schedule -- a sorted list of (I, J) per column pair, 0.4 M entries on the L1723 shape -- are built
  // by plan_stream_pairs when that schedule, the fall-back and A/B of the dataflow pass, is first used: 0.5 of this function's 0.7 ms)
  plan.h_fill = symbolic_fill(np, pair_struct); plan.stream_lists = false;
  CholTables t;
  const int64_t stored = chol_forward_lists(plan, plan.h_fill, t);
  chol_backward_lists(plan, plan.h_fill, t);
  plan.critical_pairs = chol_critical_pairs(plan, np);
  plan.dense_fraction = (double)stored / ((double)nt * (nt + 1) / 2.0);
  if (t.bwd_col_rows.empty()) t.bwd_col_rows.push_back(0);
  if (t.rows.empty()) t.rows.push_back(0);
  if (t.bcols.empty()) t.bcols.push_back(0);
  // tile -> slot (chol_device.h::SMat): the stored tiles in list order
  plan.n_stored = (int64_t)t.stored.size() / 2;
  plan.h_slot.assign((size_t)(nt + 1) * nt, -1);
  for (int64_t q = 0; q < plan.n_stored; q++) {
    int32_t& sl = plan.h_slot[(size_t)t.stored[2 * q] * nt + t.stored[2 * q + 1]];
    if (sl >= 0) throw std::runtime_error("cholesky plan: a tile is listed twice");
    sl = (int32_t)q;
  }
  return t;
}

// Per column pair p the thin update of its second column (s1), the look-ahead part of the trailing update (targets in pair p + 1:
// nar), the rest, and -- with parts -- the targets in ancestor parts (anc); every list in supertile order.
std::vector<int32_t> plan_stream_pairs(CholLists& plan) {
  const int nt = plan.nt, np = (nt + 1) / 2;
  const bool tree = !plan.pair_part.empty();
  std::vector<int32_t> pairs;
  typedef std::vector<std::pair<int32_t, int32_t>> PairList;
  auto emit_pairs = [&](PairList& v, int64_t& off, int64_t& cnt) {
    // supertile order: (J / STJ, I / STI, J % STJ, I % STI)
    std::sort(v.begin(), v.end(), [](const std::pair<int32_t, int32_t>& a, const std::pair<int32_t, int32_t>& b) {
      const int64_t ka = (((int64_t)(a.second / STJ) * 65536 + a.first / STI) * STJ + a.second % STJ) * STI + a.first % STI;
      const int64_t kb = (((int64_t)(b.second / STJ) * 65536 + b.first / STI) * STJ + b.second % STJ) * STI + b.first % STI;
      return ka < kb; });
    off = (int64_t)pairs.size() / 2; cnt = (int64_t)v.size();
    for (auto& ij : v) { pairs.push_back(ij.first); pairs.push_back(ij.second); }
  };
  std::vector<int32_t> R;
  for (int p = 0; p < np; p++) {
    const int k = 2 * p; const bool two = k + 1 < nt;
    rows_below_pair(plan.h_fill, np, nt, p, R);
    if (two) {
      PairList s1;
      s1.emplace_back(k + 1, k + 1);
      for (int32_t I : R) s1.emplace_back(I, k + 1);
      s1.emplace_back(nt, k + 1);
      emit_pairs(s1, plan.s1_off[p], plan.s1_cnt[p]);
    }
    PairList nar, rest, anc;
    for (size_t b = 0; b < R.size(); b++) {
      const int32_t J = R[b];
      // with parts: targets in another part can only be in an ancestor (no tiles between independent subtrees)
      auto& dst = (tree && plan.pair_part[J / 2] != plan.pair_part[p]) ? anc : (J / 2 == p + 1) ? nar : rest;
      for (size_t a = b; a < R.size(); a++) dst.emplace_back(R[a], J);
      dst.emplace_back(nt, J);
    }
    emit_pairs(nar, plan.nar_off[p], plan.nar_cnt[p]);
    emit_pairs(rest, plan.rest_off[p], plan.rest_cnt[p]);
    emit_pairs(anc, plan.anc_off[p], plan.anc_cnt[p]);
  }
  if (pairs.empty()) { pairs.push_back(0); pairs.push_back(0); }
  return pairs;
}

// ---- dataflow schedule ---------------------------------------------------------------------------------------------------------------
TileFill df_fill_rows(int nt, const std::vector<uint8_t>* tile_struct) {
  TileFill f;
  f.nt = nt; f.bw = (nt + 63) / 64;
  f.B = symbolic_fill(nt, tile_struct);
  f.rowcols.resize(nt);
  f.rowbits.assign((size_t)nt * f.bw, 0);
  for (int i = 0; i < nt; i++)
    for (int k = 0; k < i; k++) if (f.B[(size_t)i * nt + k]) { f.rowcols[i].push_back(k); f.rowbits[(size_t)i * f.bw + (k >> 6)] |= 1ull << (k & 63); }
  return f;
}

// ---- elimination-tree parallelism: several diagonal chains --------------------------------------------------------
// With a nested-dissection ordering (analysis.hip) the block columns fall into PARTS: leaves that do not touch each other and the
// separators above them (part_parent; children are numbered before their parent, a part is a contiguous range of tiles).  The
// reference eliminates independent subtrees of its junction tree concurrently (inference/ClusterTree-inst.h:218-317,
// base/treeTraversal/parallelTraversalTasks.h:35-156); here every leaf gets its own chain of diagonal tiles:
//   * the block columns are taken in an order `seq` that interleaves the parts that are ready (all children done) column by
//     column, pos[c] = place of column c in it.  Ticket order, contraction lists and the placement of early pieces below are all
//     stated in terms of pos (without parts pos[c] = c and everything is what it was);
//   * the chain kernel runs 2 workgroups per SLOT (<= 4 slots on the 8 reserved CUs); a leaf takes the next slot round robin,
//     a separator the slot of its first child; a slot's tiles are taken in pos order, alternating between its two workgroups.
// Deadlock freedom is unchanged: a task only waits for tasks with smaller tickets and for diagonal tiles whose own inputs have
// smaller tickets; a chain workgroup walks its tiles in pos order, so the tile it waits for is always the one whose inputs come first.
ColumnOrder df_column_sequence(int nt, const std::vector<int32_t>* tile_part, const std::vector<int32_t>* part_parent) {
  ColumnOrder o;
  o.tree = tile_part && part_parent && part_parent->size() > 1 && (int)tile_part->size() == nt;
  o.nparts = o.tree ? (int)part_parent->size() : 1;
  o.part_of.assign(nt, 0); o.pos.assign(nt, 0);
  if (o.tree) for (int c = 0; c < nt; c++) o.part_of[c] = (*tile_part)[c];
  std::vector<std::vector<int32_t>> cols(o.nparts);
  for (int c = 0; c < nt; c++) cols[o.part_of[c]].push_back(c);
  std::vector<int> pending(o.nparts, 0), next(o.nparts, 0);
  if (o.tree) for (int x = 0; x < o.nparts; x++) if ((*part_parent)[x] >= 0) pending[(*part_parent)[x]]++;
  std::vector<int> active;
  for (int x = 0; x < o.nparts; x++) if (pending[x] == 0) active.push_back(x);
  while (!active.empty()) {
    std::vector<int> still;
    for (int x : active) {
      if (next[x] < (int)cols[x].size()) o.seq.push_back(cols[x][next[x]++]);
      if (next[x] < (int)cols[x].size()) { still.push_back(x); continue; }
      const int par = o.tree ? (*part_parent)[x] : -1;
      if (par >= 0 && --pending[par] == 0) still.push_back(par);
    }
    active.swap(still);
  }
  if ((int)o.seq.size() != nt) throw std::runtime_error("dataflow plan: the parts do not cover the block columns");
  for (int q = 0; q < nt; q++) o.pos[o.seq[q]] = q;
  return o;
}

void df_chain_lists(DfLists& df, const ColumnOrder& o, const std::vector<int32_t>* part_parent) {
  const int nt = (int)o.seq.size();
  std::vector<int> slot(o.nparts, 0);
  int nslots = 1;
  if (o.tree) {
    // (round 4: 8 slots = 16 reserved CUs by default -- with the accumulator lanes of the separators' diagonal tiles in place the leaf
    // chains are the critical path of a pose graph, and they run side by side; up to 16 slots = 32 reserved CUs on request)
    // (16 slots = 32 reserved CUs since round 6: one slot per leaf of a 4-level dissection with room to spare; measured against 8 / 12
    // slots, profiles/r06j_slots_sweep.txt: sphere2500 0.913 / 0.892 / 0.892 ms, w20000 2.71 / 2.78 / 2.58 ms -- the pose graphs' bulk
    // work is a few GFLOP, the CUs cost nothing; what bounds them is the serial top of the tree, profiles/r06k_trace_sphere2500.json)
    constexpr int max_slots = 16;
    std::vector<int> first_child(o.nparts, -1);
    for (int x = o.nparts - 1; x >= 0; x--) if ((*part_parent)[x] >= 0) first_child[(*part_parent)[x]] = x;
    int leaves = 0;
    for (int x = 0; x < o.nparts; x++) if (first_child[x] < 0) slot[x] = leaves++ % max_slots;
    for (int x = 0; x < o.nparts; x++) if (first_child[x] >= 0) slot[x] = slot[first_child[x]];   // (children precede their parent)
    nslots = std::min(leaves, max_slots);
  }
  std::vector<std::vector<int32_t>> per_slot(nslots);
  for (int q = 0; q < nt; q++) per_slot[slot[o.part_of[o.seq[q]]]].push_back(o.seq[q]);      // pos order
  df.h_chain_off.assign(1, 0); df.h_chain_tiles.clear();
  const int per = nt > 1 ? 2 : 1;
  int longest = 0;
  for (int sl = 0; sl < nslots; sl++) {
    longest = std::max(longest, (int)per_slot[sl].size());
    for (int w = 0; w < per; w++) {
      for (size_t i = w; i < per_slot[sl].size(); i += per) df.h_chain_tiles.push_back(per_slot[sl][i]);
      df.h_chain_off.push_back((int32_t)df.h_chain_tiles.size());
    }
  }
  df.n_chain = (int)df.h_chain_off.size() - 1;
  df.h_seq = o.seq;
  df.critical_tiles = longest;
}

namespace {

// A tile's contraction is serial on one CU (14 us per step, up to ~30 steps) and the workgroups in flight cover only ~9 block
// columns: a long contraction taken when its column comes up would not be done when the column's diagonal tile is factored.
// So a long list is cut into PIECES of at most kPiece steps; piece r accumulates in place (tile -= its steps, flag
// part_flag = kPieceBase epoch + r + 1) and is queued EARLIER than the tile's own column: right behind the block column of its
// youngest operand, where everything it reads is final and it runs without waiting.  Only the last piece (the youngest
// kFinal steps + the substitution) sits in the tile's column and streams behind the columns before it.
// (kPiece, kFinal) swept on the L1723 shape in round 4 (Cholesky ms): (6,3) 5.17, (4,4) 5.09, (6,4) 5.10, (4,5) 5.11, (3,4) 5.14,
// (4,3) 5.15, (4,6) 5.16, (8,3) 5.32, (2,4) 5.32, (6,2) 5.48, (10,3) 5.51.
constexpr int kPiece = 4, kFinal = 4;
// The DIAGONAL tile's last piece is shorter: PD(J) is on the serial chain -- the chain workgroup of tile J cannot start before it -- and a
// last piece of 4 steps is 72 us of contraction (18 us per step) that only starts when a workgroup takes its ticket.  Round 5 trace
// (profiles/r05f_late_pd.txt): on 13 of 120 block columns of the L1723 shape the ticket was taken 53 - 74 us before the tile was needed
// instead of the usual 77 - 120, PD(J) came 7 - 20 us late, and those 13 periods (57 us instead of 41) were 0.27 ms of the 5.05.
// The same holds for the tiles right below it: (J + 1, J) feeds the next diagonal tile through the chain kernel, (J + 2, J) is the youngest
// operand of PD(J + 2) AND of the critical tile (J + 2, J + 1) -- when its last piece was taken 40 - 60 us before its column's diagonal
// tile was out (normally: 100), it was final 25 us late and both were late with it -- and (J + 3, J) is the youngest operand of that one.
// Swept on the L1723 shape (profiles/r05_plan_cut_sweep.txt; Cholesky ms): last piece of the diagonal tile 1 / 2 / 3 / 4 steps 5.17 / 5.04 / 5.03 /
// 5.09; short pieces + pulled for 0 / 2 / 3 rows below it 5.07 / 5.03 / 5.00.
#ifndef GT_DF_FINAL_DIAG
#define GT_DF_FINAL_DIAG 2
#endif
#ifndef GT_DF_NEAR_ROWS
#define GT_DF_NEAR_ROWS 3
#endif
constexpr int kFinalDiag = GT_DF_FINAL_DIAG, kNearRows = GT_DF_NEAR_ROWS;

// Cuts one tile's contraction list into pieces and files them by ticket group (df_contraction_pieces calls it tile by tile).
struct PieceCutter {
  const ColumnOrder& o;
  std::vector<int32_t>& klist;
  Pieces& out;
  std::vector<int> cut;   // (scratch) piece r = steps [cut[r], cut[r + 1])

  void emit(int I, int J, std::vector<int32_t>& ks) {
    const std::vector<int32_t>& pos = o.pos;
    if (o.tree) std::sort(ks.begin(), ks.end(), [&](int32_t a, int32_t b) { return pos[a] < pos[b]; });   // the steps in the order in which their operands come into being
    const int n = (int)ks.size(), G = pos[J];
    const bool near = I - J <= kNearRows;              // the diagonal tile and the kNearRows tiles below it: on or next to the serial chain
    int m = std::max(0, n - (near ? kFinalDiag : kFinal));   // older steps, in early pieces of at most kPiece; the last piece: the youngest
    while (m > 0 && pos[ks[m - 1]] > G - 3) m--;     // (an early piece sits two groups before its tile's column at the latest)
    const int f = n - m;
    // the early steps cut into pieces of kPiece from the old end; a DIAGONAL tile's last early piece is short as well (kFinalDiag steps):
    // the last piece cannot start before it is done, and 4 steps are 73 us (round 5 trace: PD(J) late whenever that piece had 4)
    cut.clear();
    {
      const int tail = (near && m > kFinalDiag) ? kFinalDiag : 0;
      for (int b = 0; b < m - tail; b += kPiece) cut.push_back(b);
      if (tail) cut.push_back(m - tail);
      cut.push_back(m);
    }
    const int R = (int)cut.size();     // early pieces + the last one
    if (R >= (int)kPieceBase) throw std::runtime_error("dataflow plan: a contraction list needs more pieces than the part flags can count");
    const int32_t off = (int32_t)klist.size();
    klist.insert(klist.end(), ks.begin(), ks.end());
    int gprev = 0;
    for (int r = 0; r + 1 < R; r++) {
      const int b = cut[r], e = cut[r + 1];
      const int last_k = ks[e - 1];
      const int g = std::max(pos[last_k] + 1, gprev);   // as early as its operands exist (<= G - 2)
      out.early[g].push_back(PieceRec{I, J, off + b, e - b, r, R}); gprev = g;
      if (I == J) out.diag_last_g[J] = g;
    }
    out.finals[G].push_back(PieceRec{I, J, off + m, f, R - 1, R});
  }
};

}  // namespace

Pieces df_contraction_pieces(DfLists& df, const TileFill& fill, const ColumnOrder& order) {
  const int nt = fill.nt, bw = fill.bw;
  const std::vector<std::vector<int32_t>>& rowcols = fill.rowcols;
  Pieces P;
  P.finals.resize(nt); P.early.resize(nt); P.diag_last_g.assign(nt + 1, -1);
  df.h_klist.clear();
  { size_t tiles = 0; for (int i = 0; i < nt; i++) tiles += rowcols[i].size();       // (room up front: a tile has a last piece and ~ a piece per 4 steps)
    for (int g = 0; g < nt; g++) { P.finals[g].reserve(rowcols[g].size() + nt / 2 + 4); P.early[g].reserve(2 * (tiles / nt + 1) + 16); }
    df.h_klist.reserve(16 * tiles); }
  PieceCutter cutter{order, df.h_klist, P, {}};
  double flops = 0.0; int64_t stored = 0;
  std::vector<int32_t> ks;
  df.h_has_sub.assign(nt, 0);
  for (int J = 0; J < nt; J++) {
    // the contribution of block column J-1 to the diagonal tile is applied by k_df_chain itself (streamed): not in PD's list
    ks = rowcols[J];
    if (!ks.empty() && ks.back() == J - 1) { ks.pop_back(); df.h_has_sub[J] = 1; }
    cutter.emit(J, J, ks);
    flops += kTile3 / 3.0 + (double)rowcols[J].size() * kTile3; stored++;
    for (int I = J + 1; I < nt; I++) {
      if (!fill.B[(size_t)I * nt + J]) continue;
      ks.clear();
      for (int w = 0; w < bw; w++) {
        uint64_t both = fill.rowbits[(size_t)I * bw + w] & fill.rowbits[(size_t)J * bw + w];
        while (both) { ks.push_back(64 * w + __builtin_ctzll(both)); both &= both - 1; }
      }
      cutter.emit(I, J, ks);
      flops += kTile3 + (double)ks.size() * 2.0 * kTile3; stored++;
    }
    ks = rowcols[J];
    cutter.emit(nt, J, ks);   // rhs row: y_J (flops not counted, as in the right-looking plan)
  }
  df.nt = nt;
  df.flops = flops; df.dense_fraction = (double)stored / ((double)nt * (nt + 1) / 2.0);
  if (df.h_klist.empty()) df.h_klist.push_back(0);
  return P;
}

// Ticket order: the own tasks of the column in place q (diagonal accumulation, the tile below it, ...), then the early pieces whose
// youngest operand is in place q - 2: the latency-critical tasks of a column are taken a whole group of background work ahead of the
// pieces that merely have to be done some columns later (with the early pieces of group q - 1 in front of them, the diagonal
// accumulation was taken 30 us before it was needed and the chain waited 20 us for it every few columns).
void df_ticket_order(DfLists& df, const Pieces& P, bool tree) {
  const int nt = (int)P.finals.size();
  const std::vector<std::vector<PieceRec>>& finals = P.finals; const std::vector<std::vector<PieceRec>>& early = P.early;
  df.h_tasks.clear();
  { size_t recs = 0; for (int g = 0; g < nt; g++) recs += finals[g].size() + early[g].size(); df.h_tasks.reserve(6 * recs); }
  auto put1 = [&](const PieceRec& t) { const int32_t f[6] = {t.I, t.J, t.koff, t.kcnt, t.r, t.R}; df.h_tasks.insert(df.h_tasks.end(), f, f + 6); };
  auto put = [&](const std::vector<PieceRec>& v) { for (const PieceRec& t : v) put1(t); };
  // One chain: the two tasks of a column that the serial chain waits for -- PD(J) and the tile right below the diagonal tile -- are
  // queued one group EARLIER than the rest of their column, in front of the previous group's burst of early pieces (and behind their
  // own early pieces of that burst, so that a task still only waits for smaller tickets).  A burst is several hundred pieces of
  // ~100 us: behind it PD(J) was taken 12 - 30 us too late on every sixth column of the L1723 shape and the chain period stretched
  // from 40 to 60 - 76 us (round 4 trace: 19 of 121 periods, 0.4 ms of 5.2).  Taken early the two tasks just hold two of the 248
  // workgroups a period longer.
  // (pulled with the diagonal tile: the kNearRows tiles below it; measured on L1723 in round 4, with last pieces of 4 steps everywhere: 0 rows
  // below 5.17 ms, 1 row 5.17, 3 rows 5.19; no pulling at all 5.30)
  const int pull_rows = tree ? -1 : kNearRows;
  const bool pull = pull_rows >= 0;
  auto critical = [&](const PieceRec& t, int c) { return t.J == c && t.I >= c && t.I <= c + pull_rows && t.I < nt; };
  // PD(c) itself goes one group further ahead (round 5): its last piece -- two contraction steps, 36 us, the second one streaming behind the
  // substitution of tile (c, c - 2) -- was still taken only 20 - 25 us before the chain needed it on some columns of the L1723 shape
  // (230 tickets behind the tile (c, c - 1) of the group before: profiles/r05i trace).  Allowed when all its early pieces sit in groups
  // <= q - 1 (they are queued in front of it then: a task still only waits for smaller tickets; its operand tiles (c, c - 3), (c, c - 2)
  // belong to columns <= q, whose own tasks are queued by then).
  std::vector<char> pulled(nt + 1, 0), pd_out(nt + 2, 0);
  auto is_pd = [&](const PieceRec& t, int c) { return t.I == c && t.J == c; };
  for (int q = 0; q < nt; q++) {
    for (const PieceRec& t : finals[q]) { if (pulled[q] && critical(t, q)) continue; put1(t); }
    if (q >= 1) {
      const int c = q + 1, c2 = q + 2;            // the columns whose critical tasks are pulled in front of early[q - 1]
      if (pull && c < nt) {
        const bool pd2 = c2 < nt && P.diag_last_g[c2] <= q - 1;
        for (const PieceRec& t : early[q - 1]) if (critical(t, c) || (pd2 && is_pd(t, c2))) put1(t);
        for (const PieceRec& t : finals[c]) if (critical(t, c) && !(is_pd(t, c) && pd_out[c])) put1(t);
        pulled[c] = 1;
        if (pd2) { for (const PieceRec& t : finals[c2]) if (is_pd(t, c2)) put1(t); pd_out[c2] = 1; }
        for (const PieceRec& t : early[q - 1]) if (!(critical(t, c) || (pd2 && is_pd(t, c2)))) put1(t);
      } else put(early[q - 1]);
    }
  }
  put(early[nt - 1]);
  df.n_tasks = (int64_t)df.h_tasks.size() / 6;
}

void plan_dataflow(DfLists& df, int nt, const std::vector<uint8_t>* tile_struct,
                   const std::vector<int32_t>* tile_part, const std::vector<int32_t>* part_parent) {
  const bool sect_on = std::getenv("GTG_DF_PLAN_TIMING") != nullptr;
  auto sect_t = std::chrono::high_resolution_clock::now();
  auto sect = [&](const char* what) { if (!sect_on) return; const auto n = std::chrono::high_resolution_clock::now(); std::fprintf(stderr, "[df plan] %-28s %7.3f ms\n", what, std::chrono::duration<double, std::milli>(n - sect_t).count()); sect_t = n; };
  const TileFill fill = df_fill_rows(nt, tile_struct);
  sect("symbolic fill + row lists");
  const ColumnOrder order = df_column_sequence(nt, tile_part, part_parent);
  df_chain_lists(df, order, part_parent);
  sect("parts, chains");
  const Pieces pieces = df_contraction_pieces(df, fill, order);
  sect("contraction lists, pieces");
  df_ticket_order(df, pieces, order.tree);
  sect("ticket order");
}

// ---- resolved to slots -----------------------------------------------------------------------------------------------------------------
// Device form: tiles AND their flag words are addressed by SLOT (context.h::SMat; the slots come from the stream schedule's plan,
// whose stored set -- fill at the granularity of column pairs -- contains this one).  A task carries the slots of its tile and of
// its diagonal tile, a contraction step the slots of its two operand tiles; h_tasks / h_klist keep the tile coordinates (debug
// getters, tests/test_chol_plan.py).
namespace {

int32_t slot_of(const std::vector<int32_t>& slot, int nt, int I, int J) {
  const int32_t q = slot[(size_t)I * nt + J];
  if (q < 0) throw std::runtime_error("dataflow plan: a tile of the task list has no slot in the stored-tile list");
  return q;
}
// sub-tile masks of a contraction step's operand tiles (analysis.hip: strip-level symbolic factorisation; none = every sub-tile): the
// right-hand-side row has one row of sub-tiles
uint64_t mask_of(const std::vector<uint64_t>* sub16, int nt, int I, int k) { return I >= nt ? 0xFFull : sub16 ? (*sub16)[(size_t)I * nt + k] : ~0ull; }
void push_mask(std::vector<int32_t>& v, uint64_t m) { v.push_back((int32_t)(uint32_t)m); v.push_back((int32_t)(uint32_t)(m >> 32)); }

}  // namespace

std::vector<int32_t> df_lane_table(DfLists& df, const std::vector<int32_t>& slot, int64_t n_slots) {
  // accumulator lanes of the tiles with very long contraction lists (chol_dataflow.hip::run_task): G - 1 scratch slots each, behind the stored tiles
  constexpr int lane_min = 8;   // early pieces from which a tile gets lanes
  constexpr int lane_max = 8;
  std::vector<int32_t> lane_tab(2 * (size_t)n_slots);
  for (int64_t q = 0; q < n_slots; q++) { lane_tab[2 * q] = 1; lane_tab[2 * q + 1] = -1; }
  df.n_scratch = 0;
  for (int64_t t = 0; t < df.n_tasks; t++) {
    const int32_t* d = df.h_tasks.data() + 6 * t;
    const int E = d[5] - 1;
    if (d[4] != d[5] - 1 || E < lane_min || lane_max < 2) continue;       // (looked at once per tile: at its final piece)
    const int G = std::min(lane_max, E / 4);
    if (G < 2) continue;
    const size_t q = (size_t)slot_of(slot, df.nt, d[0], d[1]);
    lane_tab[2 * q] = G; lane_tab[2 * q + 1] = (int32_t)(n_slots + df.n_scratch);
    df.n_scratch += G - 1;
  }
  return lane_tab;
}

DfTables df_resolve_host(const DfLists& df, const std::vector<int32_t>& slot, const std::vector<uint64_t>* sub16, const std::vector<int32_t>& lane_tab) {
  const int nt = df.nt;
  DfTables out;
  out.tasks.reserve((size_t)df.n_tasks * kTaskWords);
  out.steps.assign(kStepWords * df.h_klist.size(), 0);
  std::vector<uint8_t> seen(df.h_klist.size(), 0);
  for (int64_t t = 0; t < df.n_tasks; t++) {
    const int32_t* d = df.h_tasks.data() + 6 * t;
    const int I = d[0], J = d[1];
    const int32_t q = slot_of(slot, nt, I, J);
    out.tasks.insert(out.tasks.end(), d, d + 6);
    out.tasks.push_back(q); out.tasks.push_back(slot_of(slot, nt, J, J));
    out.tasks.push_back(lane_tab[2 * (size_t)q]); out.tasks.push_back(lane_tab[2 * (size_t)q + 1]);
    push_mask(out.tasks, I == J ? ~0ull : mask_of(sub16, nt, I, J));   // sub-tile mask of the tile itself (substitute)
    for (int32_t e = d[2]; e < d[2] + d[3]; e++) {   // (the pieces of a tile share one list: every entry is visited once)
      const int k = df.h_klist[e];
      int32_t* w = out.steps.data() + kStepWords * (size_t)e;
      const uint64_t ma = mask_of(sub16, nt, I, k), mb = mask_of(sub16, nt, J, k);
      w[0] = slot_of(slot, nt, I, k); w[1] = slot_of(slot, nt, J, k);
      w[2] = (int32_t)(uint32_t)ma; w[3] = (int32_t)(uint32_t)(ma >> 32); w[4] = (int32_t)(uint32_t)mb; w[5] = (int32_t)(uint32_t)(mb >> 32);
      if (!seen[e]) {   // MFMAs the step leaves out: per 16-column strip (row tiles with a live A sub-tile) x (column tiles with a live B sub-tile), 4 each
        int live = 0;
        for (int sp = 0; sp < 8; sp++) live += 4 * __builtin_popcountll(ma & (0x0101010101010101ull << sp)) * __builtin_popcountll(mb & (0x0101010101010101ull << sp));
        const int rows = I >= nt ? 1 : 8;   // (the flop count has always taken the right-hand-side row as a full tile row; its 7 idle row tiles are not counted as skipped work here)
        out.skipped += (I == J ? 0.5 : 1.0) * (double)(4 * 8 * rows * 8 - live) * 2048.0 * (I >= nt ? 0.0 : 1.0);
      }
      seen[e] = 1;
    }
  }
  return out;
}

std::vector<int32_t> df_chain_words(const DfLists& df, const std::vector<int32_t>& slot, const std::vector<uint64_t>* sub16) {
  const int nt = df.nt;
  std::vector<int32_t> cs(kChainWords * (size_t)nt, -1);
  for (int J = 0; J < nt; J++) {
    cs[kChainWords * J] = slot_of(slot, nt, J, J);
    if (df.h_has_sub[J] & 1) {
      cs[kChainWords * J + 1] = slot_of(slot, nt, J, J - 1);
      const uint64_t m = mask_of(sub16, nt, J, J - 1);
      cs[kChainWords * J + 2] = (int32_t)(uint32_t)m; cs[kChainWords * J + 3] = (int32_t)(uint32_t)(m >> 32);
    }
  }
  return cs;
}

}  // namespace gt
