// tree_export.hpp — search trees leave the device in a CANONICAL form (gaz_engine_read_trees, gaz_engine_read_pv; DESIGN.md "Reading
// search trees back"): what the reference keeps as Python objects under MCTS.root (Node.children / child_visits / child_values /
// child_prob_priors / is_terminal, MCTS.py:20-72; terminal children MCTS.py:403-426), for any number of games at once.
//
// The export is the breadth-first walk compact_subtree makes on a re-root (puct_core.hpp), READ-ONLY: from TreeState::root, parents in export
// order, the children of a node in slot order.  Export indices therefore depend on the tree alone — not on the arena index a record happens
// to have (leaf_batch / gumbel_batch allocate in another order), not on which half a compaction left it in, not on a stale header of a
// re-rooted node.  Nothing here writes the arena, a TreeState or a GameState.
//
// One TEAM of lanes per requested tree, the launch shape of k_wave_lb: a wavefront for Gomoku, a 16-lane row for Connect4 / TicTacToe.  The
// team's lanes fan out over the child slots of the node at the head of the queue: a ballot over "this child is exported" ranks the new
// nodes in slot order, and every lane writes the edge record of its slot.  The walk runs twice per call — once counting (nothing
// written but the queue), once writing at the offsets the host made of the counts.  The queue (arena index, depth per exported node)
// is scratch the host sizes from the requested trees' own node counts.
#pragma once
#include "../../include/gaz_engine.h"
#include "gumbel_core.hpp"

namespace gaz {

struct ExportQ { int32_t node, depth; };             // exported node k of a tree: its record in the arena, its depth

struct TreeExportArgs {
    const int32_t* slots; int32_t n_slots;            // requested games (host-checked: in [0, n_games))
    int32_t tree, max_depth; uint32_t min_visits;     // gaz_engine_read_trees arguments
    ExportQ* queue; const long long* q_first;         // queue of tree i: [q_first[i], q_first[i + 1]) — its TreeState::n_nodes entries
    long long* counts;                                // counting pass: [n_slots][2] nodes, edges
    const long long* node_first; const long long* edge_first;   // writing pass: [n_slots + 1] prefix sums of the counts
    gaz_tree_node* nodes; gaz_tree_edge* edges;
};

// tree = 0 / 1, or -1 = the tree running the game's move; engines with one tree per game (single_tree, Gumbel search) only have tree 0.
// Per LANE: k_tree_caps calls it with a game per lane, so nothing here may be made wave-uniform (the team kernels read one game per team
// and every lane of the team gets the same answer anyway)
template <class G> GAZ_DEV int export_tree_id(const DevParams<G>& E, int g, int tree) {
    if (E.gstate || E.single_tree) return 0;
    if (tree >= 0) return tree & 1;
    return E.games[g].runner == 1 ? 1 : 0;
}

// the node records a tree has allocated = the most its export can hold (0: no root yet)
template <class G> GAZ_KERNEL_WIDE k_tree_caps(DevParams<G> E, const int32_t* slots, int n_slots, int tree, int32_t* cap) {
#ifdef GAZ_HOST_EMU
    const int i = block_id();
#else
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
#endif
    if (i >= n_slots) return;
    const int g = slots[i];
    if (g < 0 || g >= E.n_games) { cap[i] = 0; return; }
    const TreeState& ts = E.trees[(size_t)g * 2 + export_tree_id<G>(E, g, tree)];
    const uint32_t n = ts.n_nodes < (uint32_t)E.nodes_per_tree ? ts.n_nodes : (uint32_t)E.nodes_per_tree;
    cap[i] = ts.root >= 0 ? (int32_t)n : 0;
}

// the walk of requested tree i.  WRITE = false: counts[i] = {nodes, edges}.  WRITE = true: the records, inside the tree's ranges only
template <class G, bool WRITE> GAZ_DEV void export_tree(const DevParams<G>& E, const TreeExportArgs& X, int i) {
    const int g = X.slots[i];
    if (g < 0 || g >= E.n_games) { if (!WRITE && tlane<G>() == 0) { X.counts[2 * i] = 0; X.counts[2 * i + 1] = 0; } return; }
    const int t = tuni<G>(export_tree_id<G>(E, g, X.tree));               // (one game per team here)
    const TreeState& ts = E.trees[(size_t)g * 2 + t];
    const int root = tuni<G>(ts.root);
    ExportQ* q = X.queue + X.q_first[i];
    const int qcap = (int)(X.q_first[i + 1] - X.q_first[i]);
    gaz_tree_node* on = nullptr; gaz_tree_edge* oe = nullptr;
    long long nn = 0, ne = 0;                                             // this tree's ranges of the output
    if (WRITE) { on = X.nodes + X.node_first[i]; nn = X.node_first[i + 1] - X.node_first[i]; oe = X.edges + X.edge_first[i]; ne = X.edge_first[i + 1] - X.edge_first[i]; }
    int n_new = 0; long long e_run = 0;
    if (root >= 0 && root < E.nodes_per_tree && qcap > 0) {
        if (tlane<G>() == 0) {
            q[0].node = root; q[0].depth = 0;
            if (WRITE && nn > 0) { on[0].parent = -1; on[0].slot = 0; on[0].depth = 0; }
        }
        n_new = 1;
        for (int k = 0; k < n_new; ++k) {
            wave_sync();
            const int idx = tuni<G>(q[k].node), depth = tuni<G>(q[k].depth);
            const NodeRef<G> nd = node_at(E, g, t, idx);
            const NodeHdr h = *nd.hdr();
            int na = tuni<G>((int)h.n_actions);
            if (na > G::A) na = G::A;
            if (WRITE && tlane<G>() == 0 && k < nn) {
                gaz_tree_node& o = on[k];
                o.edge0 = (int32_t)e_run; o.n_actions = na; o.n_children = h.n_children; o.flags = h.flags; o.n_reserved = (int32_t)h.pad[0];
                o.player = h.player; o.action = h.action; o.n_hist = h.n_hist; o.reserved_ = 0;
            }
            const bool deeper = X.max_depth < 0 || depth < X.max_depth;
            for (int base = 0; base < na; base += G::TEAM) {
                const int s = base + tlane<G>();
                const bool in = s < na;
                const int c = in ? child_index(nd.child()[s]) : CHILD_NONE;       // (solver: a child word may carry tag bits, tree.hpp)
                const uint32_t n = in ? nd.N()[s] : 0u;
                const bool has = in && c >= 0;
                const bool take = has && deeper && n >= X.min_visits && c < E.nodes_per_tree;
                const uint64_t m = tballot<G>(take);
                int oc = has ? (int)GAZ_TREE_CHILD_FILTERED : c;
                if (take) {
                    const int e = n_new + popcll(m & ((1ull << tlane<G>()) - 1ull));     // export index: slot order
                    if (e < qcap) {
                        q[e].node = c; q[e].depth = depth + 1; oc = e;
                        if (WRITE && e < nn) { on[e].parent = k; on[e].slot = s; on[e].depth = depth + 1; }
                    }
                }
                if (WRITE && in && e_run + s < ne) {
                    gaz_tree_edge& o = oe[e_run + s];
                    o.action = nd.act()[s]; o.N = n; o.W = nd.W()[s]; o.P = nd.P()[s]; o.raw = E.gstate ? node_raw<G>(nd)[s] : 0.0f; o.child = oc;
                }
                n_new += popcll(m);
                if (n_new > qcap) n_new = qcap;
            }
            e_run += na;
        }
    }
    if (!WRITE && tlane<G>() == 0) { X.counts[2 * i] = n_new; X.counts[2 * i + 1] = e_run; }
}

template <class G, bool WRITE> GAZ_KERNEL_TEAMS k_tree_export(DevParams<G> E, TreeExportArgs X) {
    constexpr int PER = WAVE / G::TEAM;
    const int i = block_id() * PER + team_in_wave<G>();
    if (i < X.n_slots) export_tree<G, WRITE>(E, X, i);
}

// principal variation of every game: from the root along the most visited edge (ties: the lowest slot); first_action[g] >= 0 names the
// first step.  A step records the edge's action, N and W; the line ends after an edge whose child is terminal, not expanded or unvisited
template <class G> GAZ_KERNEL_TEAMS k_tree_pv(DevParams<G> E, int tree, const int32_t* first_action, int max_len, uint8_t* o_act, uint32_t* o_N,
                                             float* o_W, int32_t* o_len) {
    constexpr int PER = WAVE / G::TEAM;
    const int g = block_id() * PER + team_in_wave<G>();
    if (g >= E.n_games) return;
    const int t = tuni<G>(export_tree_id<G>(E, g, tree));
    int node = tuni<G>(E.trees[(size_t)g * 2 + t].root);
    int len = 0;
    while (node >= 0 && node < E.nodes_per_tree && len < max_len) {
        const NodeRef<G> nd = node_at(E, g, t, node);
        int na = tuni<G>((int)nd.hdr()->n_actions);
        if (na > G::A) na = G::A;
        if (na == 0) break;
        const int fa = (len == 0 && first_action) ? tuni<G>(first_action[g]) : -1;
        int pick = -1;
        if (fa >= 0) {
            for (int base = 0; base < na && pick < 0; base += G::TEAM) {
                const int s = base + tlane<G>();
                const uint64_t m = tballot<G>(s < na && (int)nd.act()[s] == fa);          // (as int: an action index past 255 matches nothing)
                if (m) pick = base + ffsll0(m);
            }
            if (pick < 0) break;
        } else {
            uint32_t bv = 0; int bi = 0x7fffffff;
            for (int s = tlane<G>(); s < na; s += G::TEAM) { const uint32_t v = nd.N()[s]; if (bi == 0x7fffffff || v > bv) { bv = v; bi = s; } }
            team_argmax_u32<G>(bv, bi);
            pick = tuni<G>(bi);
        }
        const uint32_t pn = tuni<G>(nd.N()[pick]);
        const int c = tuni<G>(child_index(nd.child()[pick]));
        if (tlane<G>() == 0) {
            const size_t o = (size_t)g * (size_t)max_len + (size_t)len;
            o_act[o] = nd.act()[pick]; o_N[o] = pn; o_W[o] = nd.W()[pick];
        }
        len++;
        if (c < 0 || pn == 0u) break;
        node = c;
    }
    if (tlane<G>() == 0) o_len[g] = len;
}

}  // namespace gaz
