// ordering.h -- the fill-reducing order of the reduced variables and where it puts them in S: reverse Cuthill-McKee, nested
// dissection by level-set separators, plain minimum degree, the two flop counts that score them, the placement of the ordered
// variables.  Pure index arithmetic on the host, once per graph: plain C++17, nothing of the runtime, no environment, no I/O
// (ordering.cpp compiles with any host compiler; tests/cpp/test_ordering.cpp links it alone).  analysis.hip decides WHICH of these
// run (environment, sparsity criterion, device or host, the retry as one chain) and keeps everything that touches the handle.
#pragma once
#include <stdint.h>

#include <vector>

namespace gt {

// The block graph of the reduced system: node = reduced variable, edge = off-diagonal block.  a[i], b[i]: the blocks as pairs of
// reduced indices in [0, n); pairs with a[i] == b[i] are ignored, duplicates allowed.  adj: sorted, unique.
struct BlockGraph {
  std::vector<std::vector<int32_t>> adj;
  BlockGraph() = default;
  BlockGraph(int n, const std::vector<int32_t>& a, const std::vector<int32_t>& b);
};

// Reverse Cuthill-McKee of a node set, all its components (seeds in the order of `nodes`): from every seed two sweeps towards a
// pseudo-peripheral node of its component, neighbours by (degree, index), the whole visit order reversed.
std::vector<int32_t> rcm_order(const BlockGraph& g, const std::vector<int32_t>& nodes);

// Nested dissection by level-set separators, `depth` levels: the parts in elimination order (children before parents), every part's
// nodes in rcm_order.  A set of fewer than 256 nodes, or depth 0, is a leaf.  The separator is the smallest BFS level (from a
// pseudo-peripheral node) among the cuts that leave 10/20, else 8/20, else 5/20 of the nodes on each side -- nodes the BFS did not
// reach count as "above" -- and is taken only if it is smaller than a third of the set.
struct OrderingPart { std::vector<int32_t> nodes; int parent = -1; };   // parent part, -1: root
std::vector<OrderingPart> nested_dissection(const BlockGraph& g, int depth);

// The parts in a row.  part_of_pos / part_parent stay empty for exactly one part (= no parts).
struct PartOrder { std::vector<int32_t> order, part_of_pos, part_parent; };   // order: position -> reduced index
PartOrder flatten_parts(const std::vector<OrderingPart>& parts);

// Plain minimum degree on the elimination graph (ties: lowest index): what COLAMD approximates.
std::vector<int32_t> min_degree_order(const BlockGraph& g);

// Flops of the symbolic factorisation at the granularity of the variables (d x d blocks, fill included): sum over block columns of
// f^3/3 + f^2 s + f s^2, f = the variable's dimension, s = the dimension of its below-diagonal structure.  Blocks as for BlockGraph;
// order: position -> reduced index; dims by reduced index.
double block_level_flops(const std::vector<int32_t>& a, const std::vector<int32_t>& b, const std::vector<int32_t>& order, const std::vector<int32_t>& dims);

// Flops over the tile x tile tiles an ordering would store, fill included (no pad rows: the variables back to back).
double tile_level_flops(const BlockGraph& g, const std::vector<int32_t>& order, const std::vector<int32_t>& dims, int tile);

// Where the ordered variables sit in S.  Every part starts on a 2 * tile boundary (a pair of block columns belongs to one part); the
// end is aligned to tile without parts, to 2 * tile with parts.  pad: the rows / columns in between, ascending.
struct Placement { std::vector<int64_t> off, pad; int64_t NP = 0; };   // off: by reduced index
Placement place_variables(const std::vector<int32_t>& order, const std::vector<int32_t>& part_of_pos, const std::vector<int32_t>& dims, int tile);

}  // namespace gt
