// cl_tree_api.cpp — a guide tree from the sequences themselves (the reference takes its guide tree from outside: README, "Guide trees must be
// generated externally").  k-mer count spectra and their weighted Jaccard similarity on the device (tree_kernels.hip), the Mash transform
// into a distance, then on the host: neighbor joining (Saitou-Nei with the Studier-Keppler Q), a midpoint root and the Newick text in the
// style of Tree::to_newick (src/tree.cpp:615-645).  Every number and tie-break is fixed so that a few lines of Python restate the result
// bit for bit: this file is built without fused multiply-adds (Makefile, FPOFF), sums run in the order written here.
// Also here: the distances an alignment implies (cl_alignment_distances over cl_induced_pairwise_stats) and the loop that rebuilds the guide tree
// from them (cl_refine_guide_tree).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "cl_internal.hpp"

int cl_kmer_shared_counts(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, int k, uint64_t* total, uint64_t* shared,
                          float* spectra_ms, float* pairs_ms);   // tree_kernels.hip

namespace {

// J = shared / union (0 when the union is empty); 1 when J = 0, +0 when J = 1, otherwise min(1, -log(2J / (1 + J)) / k)
double mash_distance(uint64_t shared, uint64_t ti, uint64_t tj, int k) {
    const uint64_t uni = ti + tj - shared;
    const double j = uni ? (double)shared / (double)uni : 0.0;
    if (j == 0.0) return 1.0;
    if (j == 1.0) return 0.0;
    return std::min(1.0, -std::log(2.0 * j / (1.0 + j)) / (double)k);
}

struct TreeEdge { uint32_t to; double len; };
using Adjacency = std::vector<std::vector<TreeEdge>>;

double nonneg(double x) { return x > 0 ? x : 0.0; }   // !(x > 0), negative zero included, becomes +0.0

void add_edge(Adjacency& adj, uint32_t a, uint32_t b, double len) {
    adj[a].push_back({b, len});
    adj[b].push_back({a, len});
}

// leaves 0 .. n-1, internal nodes n, n+1, ... in the order they are made
Adjacency neighbor_joining(const double* dist, uint32_t n) {
    const uint32_t cap = 2 * n;
    std::vector<double> d((size_t)cap * cap, 0.0);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < n; ++j) d[(size_t)i * cap + j] = dist[(size_t)i * n + j];
    auto D = [&](uint32_t a, uint32_t b) -> double& { return d[(size_t)a * cap + b]; };
    Adjacency adj(cap);
    std::vector<uint32_t> active(n);
    for (uint32_t i = 0; i < n; ++i) active[i] = i;
    uint32_t next = n;
    while (active.size() > 2) {
        const size_t r = active.size();
        std::vector<double> R(r);
        for (size_t x = 0; x < r; ++x) {
            double s = 0.0;
            for (size_t y = 0; y < r; ++y) if (y != x) s += D(active[x], active[y]);
            R[x] = s;
        }
        const double rm2 = (double)(r - 2);
        size_t bx = 0, by = 1;
        double best = 0.0;
        bool have = false;
        for (size_t x = 0; x < r; ++x)
            for (size_t y = x + 1; y < r; ++y) {
                const double q = rm2 * D(active[x], active[y]) - R[x] - R[y];
                if (!have || q < best) { best = q; bx = x; by = y; have = true; }
            }
        const uint32_t a = active[bx], b = active[by], u = next++;
        const double dab = D(a, b);
        const double la = dab / 2 + (R[bx] - R[by]) / (2 * rm2), lb = dab - la;
        for (uint32_t c : active)
            if (c != a && c != b) D(u, c) = D(c, u) = (D(a, c) + D(b, c) - dab) / 2;
        add_edge(adj, u, a, nonneg(la));
        add_edge(adj, u, b, nonneg(lb));
        active.erase(active.begin() + by);
        active.erase(active.begin() + bx);
        active.push_back(u);
    }
    add_edge(adj, active[0], active[1], nonneg(D(active[0], active[1])));
    adj.resize(next);
    return adj;
}

// path lengths from p, summed outward, and every node's neighbour toward p
void walk_from(const Adjacency& adj, uint32_t p, std::vector<double>& dist, std::vector<uint32_t>& toward) {
    dist.assign(adj.size(), 0.0);
    toward.assign(adj.size(), UINT32_MAX);
    std::vector<uint32_t> stack{p};
    toward[p] = p;
    while (!stack.empty()) {
        const uint32_t u = stack.back();
        stack.pop_back();
        for (const TreeEdge& e : adj[u])
            if (toward[e.to] == UINT32_MAX) {
                toward[e.to] = u;
                dist[e.to] = dist[u] + e.len;
                stack.push_back(e.to);
            }
    }
}

void remove_edge(Adjacency& adj, uint32_t a, uint32_t b) {
    for (uint32_t x : {a, b}) {
        auto& v = adj[x];
        const uint32_t y = x == a ? b : a;
        v.erase(std::find_if(v.begin(), v.end(), [&](const TreeEdge& e) { return e.to == y; }));
    }
}

// the midpoint of the longest leaf-to-leaf path (smallest (p, q) on a tie) becomes the root: a node of the tree, or a new one on an edge
uint32_t midpoint_root(Adjacency& adj, uint32_t n) {
    std::vector<double> dist;
    std::vector<uint32_t> toward;
    uint32_t bp = 0, bq = 1;
    double longest = 0.0;
    bool have = false;
    for (uint32_t p = 0; p < n; ++p) {
        walk_from(adj, p, dist, toward);
        for (uint32_t q = p + 1; q < n; ++q)
            if (!have || dist[q] > longest) { longest = dist[q]; bp = p; bq = q; have = true; }
    }
    walk_from(adj, bp, dist, toward);
    std::vector<uint32_t> path{bq};
    while (path.back() != bp) path.push_back(toward[path.back()]);
    std::reverse(path.begin(), path.end());   // bp .. bq
    const double half = longest / 2;
    double acc = 0.0;
    for (size_t i = 0; i + 1 < path.size(); ++i) {
        const uint32_t u = path[i], v = path[i + 1];
        if (acc == half && u >= n) return u;
        double len = 0.0;
        for (const TreeEdge& e : adj[u]) if (e.to == v) len = e.len;
        if (acc + len > half || acc == half) {   // (acc == half at a leaf: zero-length paths, the pendant edge is split at offset 0)
            const double x = half - acc;
            const uint32_t r = (uint32_t)adj.size();
            adj.emplace_back();
            remove_edge(adj, u, v);
            add_edge(adj, r, u, x);
            add_edge(adj, r, v, len - x);
            return r;
        }
        acc += len;
    }
    return bp;   // (not reached: the last edge takes acc to the full length)
}

std::string format_length(double x) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%g", x);
    return buf;
}

// Tree::to_newick: children in the order of the smallest leaf index below them, leaves quoted, every non-root node with its length
std::string to_newick(const Adjacency& adj, uint32_t root, uint32_t n, const char* const* names) {
    const size_t V = adj.size();
    std::vector<uint32_t> parent(V, UINT32_MAX), order, min_leaf(V, UINT32_MAX);
    std::vector<double> up_len(V, 0.0);
    parent[root] = root;
    order.push_back(root);
    for (size_t i = 0; i < order.size(); ++i)
        for (const TreeEdge& e : adj[order[i]])
            if (parent[e.to] == UINT32_MAX) {
                parent[e.to] = order[i];
                up_len[e.to] = e.len;
                order.push_back(e.to);
            }
    for (size_t i = order.size(); i-- > 0;) {
        const uint32_t u = order[i];
        if (u < n) min_leaf[u] = u;
        if (u != root) min_leaf[parent[u]] = std::min(min_leaf[parent[u]], min_leaf[u]);
    }
    std::vector<std::vector<uint32_t>> kids(V);
    for (uint32_t u : order) if (u != root) kids[parent[u]].push_back(u);
    for (auto& k : kids) std::sort(k.begin(), k.end(), [&](uint32_t a, uint32_t b) { return min_leaf[a] < min_leaf[b]; });
    std::string out;
    // iterative pre/post order: (node, next child to write)
    std::vector<std::pair<uint32_t, size_t>> stack{{root, 0}};
    while (!stack.empty()) {
        auto& top = stack.back();
        const uint32_t u = top.first;
        if (!kids[u].empty()) {
            if (top.second == 0) out += '(';
            if (top.second < kids[u].size()) {
                if (top.second) out += ',';
                const uint32_t c = kids[u][top.second++];
                stack.push_back({c, 0});
                continue;
            }
            out += ')';
        } else {
            out += '"';
            out += names[u];
            out += '"';
        }
        if (u != root) out += ':' + format_length(up_len[u]);
        stack.pop_back();
    }
    out += ';';
    return out;
}

char* to_c_string(const std::string& s, uint64_t* len_out) {
    char* p = (char*)malloc(s.size() + 1);
    if (!p) return nullptr;
    memcpy(p, s.data(), s.size());
    p[s.size()] = '\0';
    if (len_out) *len_out = s.size();
    return p;
}

}  // namespace

extern "C" {

void cl_kmer_distances_free(cl_kmer_distances* d) {
    if (!d) return;
    free(d->total);
    free(d->shared);
    free(d->distance);
    memset(d, 0, sizeof(*d));
}

int cl_kmer_distances_compute(cl_context* ctx, const char* const* sequences, const uint64_t* lengths, uint64_t n, int k, cl_kmer_distances* out) {
    cl_bind_device(ctx);
    if (out) memset(out, 0, sizeof(*out));
    if (!ctx || !out || (n && (!sequences || !lengths))) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    if (k < 1 || k > 31) { cl_set_error(ctx, "k must lie in 1..31, got %d", k); return CL_ERR_INVALID_ARGUMENT; }
    if (n < 2) { cl_set_error(ctx, "k-mer distances need at least 2 sequences, got %llu", (unsigned long long)n); return CL_ERR_INVALID_ARGUMENT; }
    if (n > 0xFFFFFFFFull / 2) { cl_set_error(ctx, "too many sequences: %llu", (unsigned long long)n); return CL_ERR_INVALID_ARGUMENT; }
    for (uint64_t i = 0; i < n; ++i)
        if (lengths[i] && !sequences[i]) { cl_set_error(ctx, "sequence %llu is null", (unsigned long long)i); return CL_ERR_INVALID_ARGUMENT; }
    cl_kmer_distances d;
    memset(&d, 0, sizeof(d));
    d.n = n;
    d.k = k;
    d.total = (uint64_t*)malloc(n * sizeof(uint64_t));
    d.shared = (uint64_t*)malloc(n * n * sizeof(uint64_t));
    d.distance = (double*)malloc(n * n * sizeof(double));
    if (!d.total || !d.shared || !d.distance) { cl_kmer_distances_free(&d); return CL_ERR_OUT_OF_MEMORY; }
    const int rc = cl_kmer_shared_counts(ctx, sequences, lengths, n, k, d.total, d.shared, &d.spectra_ms, &d.pairs_ms);
    if (rc) { cl_kmer_distances_free(&d); return rc; }
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t j = 0; j < n; ++j)
            d.distance[i * n + j] = i == j ? 0.0 : mash_distance(d.shared[i * n + j], d.total[i], d.total[j], k);
    *out = d;
    return CL_OK;
}

int cl_neighbor_joining_newick(const double* distance, uint64_t n, const char* const* names, char** newick_out, uint64_t* len_out) {
    if (newick_out) *newick_out = nullptr;
    if (!distance || !names || !newick_out) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    if (n < 2) { cl_set_error(nullptr, "a guide tree needs at least 2 sequences, got %llu", (unsigned long long)n); return CL_ERR_INVALID_ARGUMENT; }
    if (n > 0xFFFFFFFFull / 4) { cl_set_error(nullptr, "too many sequences: %llu", (unsigned long long)n); return CL_ERR_INVALID_ARGUMENT; }
    std::set<std::string> seen;
    for (uint64_t i = 0; i < n; ++i) {
        if (!names[i] || !*names[i]) { cl_set_error(nullptr, "sequence %llu has no name", (unsigned long long)i); return CL_ERR_INVALID_ARGUMENT; }
        if (strchr(names[i], '"')) { cl_set_error(nullptr, "Sequence names cannot have internal quotation marks: %s", names[i]); return CL_ERR_INVALID_ARGUMENT; }
        if (!seen.insert(names[i]).second) { cl_set_error(nullptr, "duplicate sequence name: %s", names[i]); return CL_ERR_INVALID_ARGUMENT; }
    }
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t j = 0; j < n; ++j) {
            const double x = distance[i * n + j];
            if (!std::isfinite(x) || x != distance[j * n + i] || (i == j && x != 0.0)) {
                cl_set_error(nullptr, "the distance matrix must be finite and symmetric with a zero diagonal (entry %llu, %llu)", (unsigned long long)i,
                             (unsigned long long)j);
                return CL_ERR_INVALID_ARGUMENT;
            }
        }
    Adjacency adj = neighbor_joining(distance, (uint32_t)n);
    const uint32_t root = midpoint_root(adj, (uint32_t)n);
    const std::string text = to_newick(adj, root, (uint32_t)n, names);
    *newick_out = to_c_string(text, len_out);
    return *newick_out ? CL_OK : CL_ERR_OUT_OF_MEMORY;
}

int cl_infer_guide_tree(cl_context* ctx, const char* fasta_text, uint64_t fasta_len, int k, char** newick_out, uint64_t* len_out) {
    cl_bind_device(ctx);
    if (newick_out) *newick_out = nullptr;
    if (!ctx || !fasta_text || !newick_out) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    cl_fasta fa;
    int rc = cl_parse_fasta(ctx, fasta_text, fasta_len, &fa);
    if (rc) return rc;
    struct FreeFasta { cl_fasta* f; ~FreeFasta() { cl_fasta_free(f); } } free_fasta{&fa};
    cl_kmer_distances d;
    if ((rc = cl_kmer_distances_compute(ctx, fa.sequences, fa.lengths, fa.n_sequences, k, &d))) return rc;
    rc = cl_neighbor_joining_newick(d.distance, d.n, fa.names, newick_out, len_out);
    cl_kmer_distances_free(&d);
    if (rc) cl_set_error(ctx, "%s", cl_last_error(nullptr));
    return rc;
}

// 1 - 2 eq / (2 eq + 2 x + ins + del): the share of the two sequences' bases outside '=' columns (this project's definition; header)
int cl_alignment_distances(const cl_pair_stats* stats, uint64_t n, double* distance_out) {
    if (!stats || !distance_out || n < 2) return CL_ERR_INVALID_ARGUMENT;
    uint64_t k = 0;
    for (uint64_t a = 0; a < n; ++a) {
        distance_out[a * n + a] = 0.0;
        for (uint64_t b = a + 1; b < n; ++b, ++k) {
            const uint64_t eq2 = 2 * stats[k].eq, den = eq2 + 2 * stats[k].x + stats[k].ins + stats[k].del;
            const double d = eq2 == den || den == 0 ? 0.0 : 1.0 - (double)eq2 / (double)den;
            distance_out[a * n + b] = distance_out[b * n + a] = d;
        }
    }
    return CL_OK;
}

int cl_refine_guide_tree(cl_context* ctx, const char* fasta_text, uint64_t fasta_len, const char* newick, const cl_msa_params* params, int max_rounds,
                         char** newick_out, uint64_t* len_out, int* rounds_run_out, int* converged_out) {
    cl_bind_device(ctx);
    if (newick_out) *newick_out = nullptr;
    if (len_out) *len_out = 0;
    if (rounds_run_out) *rounds_run_out = 0;
    if (converged_out) *converged_out = 0;
    if (!ctx || !fasta_text || !params || !newick_out) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    if (max_rounds < 1) { cl_set_error(ctx, "cl_refine_guide_tree needs at least one round, got %d", max_rounds); return CL_ERR_INVALID_ARGUMENT; }
    cl_fasta fa;
    int rc = cl_parse_fasta(ctx, fasta_text, fasta_len, &fa);
    if (rc) return rc;
    struct FreeFasta { cl_fasta* f; ~FreeFasta() { cl_fasta_free(f); } } free_fasta{&fa};
    const uint64_t n = fa.n_sequences;
    if (n < 2) { cl_set_error(ctx, "FASTA input contains %llu sequence(s), cannot form an alignment", (unsigned long long)n); return CL_ERR_INVALID_ARGUMENT; }
    bool have_tree = newick != nullptr;   // false: the in-order tree, which has no text here
    std::string current = newick ? newick : "";
    cl_msa_params mp = *params;   // the alignment of a round writes nothing but its GFA
    mp.subproblems_prefix = mp.induced_pairwise_prefix = mp.subalignments_path = mp.bonds_prefix = mp.pair_stats_path = nullptr;
    mp.restart = 0;
    mp.cyclize = 0;
    mp.force_gfa_output = 1;
    int rounds = 0, converged = 0;
    while (n >= 3 && rounds < max_rounds && !converged) {
        char* text = nullptr;
        uint64_t len = 0;
        if ((rc = cl_msa(ctx, fasta_text, fasta_len, have_tree ? current.c_str() : nullptr, &mp, &text, &len, nullptr))) return rc;
        cl_owned_base_graph* owned = nullptr;
        char** path_names = nullptr;
        uint64_t n_paths = 0;
        rc = cl_read_gfa(text, len, 1, &owned, &path_names, &n_paths);
        free(text);
        if (rc) { cl_set_error(ctx, "cannot read back the alignment of refinement round %d", rounds + 1); return rc; }
        std::vector<uint64_t> seq_of(n_paths, n);   // path -> FASTA index
        for (uint64_t p = 0; p < n_paths; ++p) {
            for (uint64_t q = 0; q < n && seq_of[p] == n; ++q) if (strcmp(fa.names[q], path_names[p]) == 0) seq_of[p] = q;
            free(path_names[p]);
        }
        free(path_names);
        struct FreeGraph { cl_owned_base_graph* g; ~FreeGraph() { cl_owned_base_graph_free(g); } } free_graph{owned};
        if (n_paths != n || std::set<uint64_t>(seq_of.begin(), seq_of.end()).size() != n || *std::max_element(seq_of.begin(), seq_of.end()) >= n) {
            cl_set_error(ctx, "the alignment of refinement round %d does not hold every sequence once", rounds + 1);
            return CL_ERR_INVALID_ARGUMENT;
        }
        cl_base_graph g;
        cl_owned_base_graph_view(owned, &g);
        std::vector<uint64_t> pairs;
        for (uint64_t p = 0; p < n; ++p)
            for (uint64_t q = p + 1; q < n; ++q) { pairs.push_back(p); pairs.push_back(q); }
        std::vector<cl_pair_stats> stats(pairs.size() / 2);
        if ((rc = cl_induced_pairwise_stats(ctx, &g, pairs.data(), stats.size(), stats.data()))) return rc;
        std::vector<double> by_path(n * n), by_seq(n * n);
        if ((rc = cl_alignment_distances(stats.data(), n, by_path.data()))) return rc;
        for (uint64_t p = 0; p < n; ++p)
            for (uint64_t q = 0; q < n; ++q) by_seq[seq_of[p] * n + seq_of[q]] = by_path[p * n + q];
        char* tree = nullptr;
        uint64_t tree_len = 0;
        if ((rc = cl_neighbor_joining_newick(by_seq.data(), n, fa.names, &tree, &tree_len))) { cl_set_error(ctx, "%s", cl_last_error(nullptr)); return rc; }
        const std::string next(tree, tree_len);
        free(tree);
        ++rounds;
        converged = have_tree && next == current;
        current = next;
        have_tree = true;
    }
    if (have_tree) {
        char* out = (char*)malloc(current.size() + 1);
        if (!out) return CL_ERR_OUT_OF_MEMORY;
        memcpy(out, current.c_str(), current.size() + 1);
        *newick_out = out;
        if (len_out) *len_out = current.size();
    }
    if (rounds_run_out) *rounds_run_out = rounds;
    if (converged_out) *converged_out = converged;
    return CL_OK;
}

}  // extern "C"
