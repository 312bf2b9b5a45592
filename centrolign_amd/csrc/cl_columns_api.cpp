// cl_columns_api.cpp — the MSA as columns (include/centrolign_amd.h, "The MSA as columns"):
//   cl_msa_column_layout     the column of every node: a Kahn pass over the path edges (host: a dependent chain as long as the graph)
//   cl_msa_columns_host      rows, column records and sites on the host: the definition
//   cl_msa_columns_compute   the same from a device tile of block_cols columns at a time (kernels: msa_columns_kernels.hip)
// Both entry points begin with the same checks and the same layout call; what differs is where the matrix is made and counted.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "cl_internal.hpp"

namespace {

constexpr uint32_t kNoCol = 0xFFFFFFFFu;
constexpr uint64_t kTileBytes = 256ull << 20;   // the device tile of the default block size
constexpr uint32_t kWantRows = 1, kWantColumns = 2, kWantSites = 4;

uint64_t n_steps_of(const cl_base_graph* g) { return g->n_paths ? g->path_off[g->n_paths] : 0; }

// what both entry points refuse before anything is computed
int check_arguments(const cl_base_graph* g, const cl_msa_columns_params* params, cl_msa_columns* out) {
    if (!g || !params || !out) return CL_ERR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    if (params->layout != 0 && params->layout != 1) return CL_ERR_INVALID_ARGUMENT;
    if (params->want & ~(kWantRows | kWantColumns | kWantSites)) return CL_ERR_INVALID_ARGUMENT;
    if (params->min_minor == 0) return CL_ERR_INVALID_ARGUMENT;
    if (g->n_paths >= 0xFFFFFFFFull) return CL_ERR_INVALID_ARGUMENT;   // the counts of a column are 32-bit
    for (uint64_t i = 0, n = n_steps_of(g); i < n; ++i)
        if (g->path_nodes[i] >= g->n_nodes || g->label[g->path_nodes[i]] > 4) return CL_ERR_INVALID_ARGUMENT;
    return CL_OK;
}

template <class T>
T* alloc_array(uint64_t n) { return (T*)malloc(std::max<uint64_t>(n, 1) * sizeof(T)); }

thread_local double tls_layout_seconds = 0.0;   // cl_msa_columns_layout_seconds

// node_col and n_cols of `out` (the layout call), after check_arguments
int layout_into(const cl_base_graph* g, const cl_msa_columns_params* params, cl_msa_columns* out) {
    out->n_paths = g->n_paths;
    if (!(out->node_col = alloc_array<uint32_t>(g->n_nodes))) return CL_ERR_OUT_OF_MEMORY;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = cl_msa_column_layout(g, params->layout, out->node_col, &out->n_cols);
    tls_layout_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

cl_msa_column column_record(const uint32_t* cnt, uint32_t n_paths, uint32_t min_minor, uint32_t max_gaps) {
    cl_msa_column r;
    uint32_t sum = 0, best = 0;
    for (int k = 0; k < 5; ++k) { r.count[k] = cnt[k]; sum += cnt[k]; }
    r.gaps = n_paths - sum;
    r.consensus = 0;
    for (uint32_t k = 0; k < 6; ++k) {
        const uint32_t c = k < 5 ? cnt[k] : r.gaps;
        if (k == 0 || c > best) { best = c; r.consensus = k; }
    }
    uint32_t acgt[4] = {cnt[0], cnt[1], cnt[2], cnt[3]};
    std::sort(acgt, acgt + 4);
    r.flags = (acgt[2] >= min_minor && r.gaps <= max_gaps ? 1u : 0u) | (r.gaps > 0 ? 2u : 0u) | (cnt[4] > 0 ? 4u : 0u);
    return r;
}

// The step range [lo, hi) of every path whose columns fall into [c0, c1): a path's columns strictly increase, so hi is found by binary search and
// is the next block's lo.  range[2p], range[2p + 1]; returns the longest range.
uint64_t block_ranges(const cl_base_graph* g, const uint32_t* node_col, uint64_t c1, std::vector<uint64_t>& next_lo, std::vector<uint64_t>& range) {
    uint64_t longest = 0;
    for (uint64_t p = 0; p < g->n_paths; ++p) {
        const uint32_t* first = g->path_nodes + next_lo[p];
        const uint32_t* last = g->path_nodes + g->path_off[p + 1];
        const uint64_t hi = next_lo[p] + (uint64_t)(std::partition_point(first, last, [&](uint32_t v) { return node_col[v] < c1; }) - first);
        range[2 * p] = next_lo[p];
        range[2 * p + 1] = hi;
        longest = std::max(longest, hi - next_lo[p]);
        next_lo[p] = hi;
    }
    return longest;
}

}  // namespace

extern "C" {

void cl_msa_columns_params_default(cl_msa_columns_params* params) {
    if (!params) return;
    params->layout = 0;
    params->want = kWantRows | kWantColumns | kWantSites;
    params->min_minor = 1;
    params->max_gaps = 0xFFFFFFFFu;
    params->block_cols = 0;
}

double cl_msa_columns_layout_seconds(void) { return tls_layout_seconds; }

void cl_msa_columns_free(cl_msa_columns* out) {
    if (!out) return;
    free(out->node_col);
    free(out->rows);
    free(out->columns);
    free(out->site_col);
    free(out->site_rows);
    memset(out, 0, sizeof(*out));
}

int cl_msa_column_layout(const cl_base_graph* g, int layout, uint32_t* node_col, uint64_t* n_cols_out) {
    if (!g || !node_col || !n_cols_out || (layout != 0 && layout != 1)) return CL_ERR_INVALID_ARGUMENT;
    *n_cols_out = 0;
    const uint64_t n = g->n_nodes, n_steps = n_steps_of(g);
    for (uint64_t i = 0; i < n_steps; ++i) if (g->path_nodes[i] >= n) return CL_ERR_INVALID_ARGUMENT;
    try {
        // the path edges as a CSR by tail node, with multiplicity: an edge two paths share is relaxed once per path
        std::vector<uint64_t> out_off(n + 1, 0);
        std::vector<uint32_t> in_deg(n, 0), level(n, 0);
        std::vector<uint8_t> used(n, 0);
        for (uint64_t p = 0; p < g->n_paths; ++p)
            for (uint64_t i = g->path_off[p]; i < g->path_off[p + 1]; ++i) {
                used[g->path_nodes[i]] = 1;
                if (i + 1 < g->path_off[p + 1]) { ++out_off[g->path_nodes[i] + 1]; ++in_deg[g->path_nodes[i + 1]]; }
            }
        for (uint64_t v = 0; v < n; ++v) out_off[v + 1] += out_off[v];
        std::vector<uint32_t> head(out_off[n]);
        {
            std::vector<uint64_t> at(out_off.begin(), out_off.end() - 1);
            for (uint64_t p = 0; p < g->n_paths; ++p)
                for (uint64_t i = g->path_off[p]; i + 1 < g->path_off[p + 1]; ++i) head[at[g->path_nodes[i]]++] = g->path_nodes[i + 1];
        }
        std::vector<uint32_t> queue;
        uint64_t n_used = 0;
        for (uint64_t v = 0; v < n; ++v) {
            n_used += used[v];
            if (used[v] && in_deg[v] == 0) queue.push_back((uint32_t)v);
        }
        uint64_t max_level = 0;
        for (size_t at = 0; at < queue.size(); ++at) {   // Kahn: a node leaves the queue once all its in-edges have been relaxed
            const uint32_t u = queue[at];
            max_level = std::max<uint64_t>(max_level, level[u]);
            for (uint64_t e = out_off[u]; e < out_off[u + 1]; ++e) {
                const uint32_t v = head[e];
                level[v] = std::max(level[v], level[u] + 1);
                if (--in_deg[v] == 0) queue.push_back(v);
            }
        }
        if (queue.size() != n_used) return CL_ERR_CYCLIC_GRAPH;
        const uint64_t n_cols = layout == 0 ? (n_used ? max_level + 1 : 0) : n_used;
        if (n_cols >= 0xFFFFFFFFull) return CL_ERR_INVALID_ARGUMENT;
        if (layout == 0) {
            for (uint64_t v = 0; v < n; ++v) node_col[v] = used[v] ? level[v] : kNoCol;
        } else {   // the used nodes ordered by (level, id): a counting sort by level, ids ascending within one
            std::vector<uint32_t> first(max_level + 2, 0);
            for (uint64_t v = 0; v < n; ++v) if (used[v]) ++first[level[v] + 1];
            for (uint64_t l = 0; l <= max_level; ++l) first[l + 1] += first[l];
            for (uint64_t v = 0; v < n; ++v) node_col[v] = used[v] ? first[level[v]]++ : kNoCol;
        }
        *n_cols_out = n_cols;
    } catch (const std::bad_alloc&) {
        return CL_ERR_OUT_OF_MEMORY;
    }
    return CL_OK;
}

int cl_msa_columns_host(const cl_base_graph* g, const cl_msa_columns_params* params, cl_msa_columns* out) {
    int rc = check_arguments(g, params, out);
    if (rc == CL_OK) rc = layout_into(g, params, out);
    if (rc) { if (out) cl_msa_columns_free(out); return rc; }
    const uint64_t P = g->n_paths, W = out->n_cols;
    const uint32_t want = params->want;
    const uint32_t* col = out->node_col;
    static const char dec[] = {'A', 'C', 'G', 'T', 'N'};
    auto oom = [&] { cl_msa_columns_free(out); return CL_ERR_OUT_OF_MEMORY; };
    if (want & kWantRows) {
        if (!(out->rows = alloc_array<char>(P * W))) return oom();
        memset(out->rows, '-', P * W);
        for (uint64_t p = 0; p < P; ++p)
            for (uint64_t i = g->path_off[p]; i < g->path_off[p + 1]; ++i) out->rows[p * W + col[g->path_nodes[i]]] = dec[g->label[g->path_nodes[i]]];
    }
    if (!(want & (kWantColumns | kWantSites))) return CL_OK;
    cl_msa_column* columns = alloc_array<cl_msa_column>(W);
    if (!columns) return oom();
    if (want & kWantColumns) out->columns = columns;
    struct FreeUnwanted { cl_msa_column* p; ~FreeUnwanted() { free(p); } } free_unwanted{want & kWantColumns ? nullptr : columns};
    try {
        std::vector<uint32_t> counts(5 * W, 0);
        for (uint64_t i = 0, n = n_steps_of(g); i < n; ++i) ++counts[5 * (uint64_t)col[g->path_nodes[i]] + g->label[g->path_nodes[i]]];
        for (uint64_t c = 0; c < W; ++c) columns[c] = column_record(&counts[5 * c], (uint32_t)P, params->min_minor, params->max_gaps);
        if (want & kWantSites) {
            std::vector<uint32_t> site_of(W, kNoCol);   // column -> its place among the sites
            uint64_t n_sites = 0;
            for (uint64_t c = 0; c < W; ++c) if (columns[c].flags & 1u) site_of[c] = (uint32_t)n_sites++;
            out->n_sites = n_sites;
            if (!(out->site_col = alloc_array<uint64_t>(n_sites)) || !(out->site_rows = alloc_array<char>(P * n_sites))) return oom();
            for (uint64_t c = 0; c < W; ++c) if (site_of[c] != kNoCol) out->site_col[site_of[c]] = c;
            memset(out->site_rows, '-', P * n_sites);
            for (uint64_t p = 0; p < P; ++p)
                for (uint64_t i = g->path_off[p]; i < g->path_off[p + 1]; ++i) {
                    const uint32_t k = site_of[col[g->path_nodes[i]]];
                    if (k != kNoCol) out->site_rows[p * n_sites + k] = dec[g->label[g->path_nodes[i]]];
                }
        }
    } catch (const std::bad_alloc&) {
        return oom();
    }
    return CL_OK;
}

static int columns_compute(cl_context* ctx, const cl_base_graph* g, const cl_msa_columns_params* params, cl_msa_columns* out);

int cl_msa_columns_compute(cl_context* ctx, const cl_base_graph* g, const cl_msa_columns_params* params, cl_msa_columns* out) {
    cl_bind_device(ctx);
    if (!ctx) return CL_ERR_INVALID_ARGUMENT;
    try {
        return columns_compute(ctx, g, params, out);
    } catch (const std::bad_alloc&) {   // (a host vector; what `out` held has been released on the way)
        return CL_ERR_OUT_OF_MEMORY;
    }
}

static int columns_compute(cl_context* ctx, const cl_base_graph* g, const cl_msa_columns_params* params, cl_msa_columns* out) {
    int rc = check_arguments(g, params, out);
    if (rc == CL_OK) rc = layout_into(g, params, out);
    if (rc) {
        if (out) cl_msa_columns_free(out);
        cl_set_error(ctx, "the MSA as columns: %s", rc == CL_ERR_CYCLIC_GRAPH ? "the path edges of the graph have a cycle" : "invalid graph or parameters");
        return rc;
    }
    const uint64_t P = g->n_paths, W = out->n_cols, n_steps = n_steps_of(g);
    const uint32_t want = params->want;
    struct FreeOnError { cl_msa_columns* out; bool keep = false; ~FreeOnError() { if (!keep) cl_msa_columns_free(out); } } guard{out};
    if ((want & kWantRows) && !(out->rows = alloc_array<char>(P * W))) return CL_ERR_OUT_OF_MEMORY;
    if ((want & kWantColumns) && !(out->columns = alloc_array<cl_msa_column>(W))) return CL_ERR_OUT_OF_MEMORY;
    std::vector<uint64_t> site_col;                 // the sites of the blocks so far
    std::vector<std::vector<char>> site_pieces;     // per block its P x (sites of the block) bytes
    std::vector<uint64_t> piece_sites;
    if (W > 0 && P > 0) {
        uint64_t block_cols = params->block_cols;
        if (block_cols == 0) block_cols = std::max<uint64_t>(256, kTileBytes / P / 256 * 256);
        block_cols = std::min(block_cols, W);
        const uint64_t stride = (block_cols + 3) / 4 * 4;
        const bool reduce = want & (kWantColumns | kWantSites);
        ScopedBuf<uint32_t> d_nodes, d_col, d_counts, d_offsets;
        ScopedBuf<uint8_t> d_label;
        ScopedBuf<uint64_t> d_range;
        ScopedBuf<char> d_tile;
        ScopedBuf<cl_msa_column> d_records;
        const uint32_t max_groups = cl_msa_site_groups((uint32_t)block_cols);
        if ((rc = d_nodes.alloc(ctx, n_steps)) || (rc = d_col.alloc(ctx, g->n_nodes)) || (rc = d_label.alloc(ctx, g->n_nodes)) || (rc = d_range.alloc(ctx, 2 * P)) ||
            (rc = d_tile.alloc(ctx, P * stride)))
            return rc;
        if (reduce && (rc = d_records.alloc(ctx, block_cols))) return rc;
        if ((want & kWantSites) && ((rc = d_counts.alloc(ctx, max_groups)) || (rc = d_offsets.alloc(ctx, max_groups)))) return rc;
        HIP_TRY(ctx, cl_copy_sync(ctx, d_nodes.p, g->path_nodes, n_steps * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(ctx, cl_copy_sync(ctx, d_col.p, out->node_col, g->n_nodes * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(ctx, cl_copy_sync(ctx, d_label.p, g->label, g->n_nodes, hipMemcpyHostToDevice));
        std::vector<uint64_t> next_lo(g->path_off, g->path_off + P), range(2 * P);
        std::vector<uint32_t> counts(max_groups);
        for (uint64_t c0 = 0; c0 < W; c0 += block_cols) {
            const uint64_t c1 = std::min(W, c0 + block_cols);
            const uint32_t width = (uint32_t)(c1 - c0), groups = cl_msa_site_groups(width);
            const uint64_t longest = block_ranges(g, out->node_col, c1, next_lo, range);
            HIP_TRY(ctx, cl_copy_sync(ctx, d_range.p, range.data(), range.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
            HIP_TRY(ctx, hipMemsetAsync(d_tile.p, '-', P * stride, ctx->stream));
            HIP_TRY(ctx, cl_launch_msa_fill(d_nodes.p, d_range.p, P, longest, d_label.p, d_col.p, (uint32_t)c0, width, stride, d_tile.p, ctx->stream));
            if (want & kWantRows)   // the block's columns of every row: a strided copy into the caller's P x W matrix
                HIP_TRY(ctx, hipMemcpy2DAsync(out->rows + c0, W, d_tile.p, stride, width, P, hipMemcpyDeviceToHost, ctx->stream));
            if (reduce) HIP_TRY(ctx, cl_launch_msa_reduce(d_tile.p, P, stride, width, params->min_minor, params->max_gaps, d_records.p, ctx->stream));
            if (want & kWantColumns) HIP_TRY(ctx, hipMemcpyAsync(out->columns + c0, d_records.p, width * sizeof(cl_msa_column), hipMemcpyDeviceToHost, ctx->stream));
            if (want & kWantSites) {
                HIP_TRY(ctx, cl_launch_msa_sites(false, d_records.p, width, d_counts.p, nullptr, c0, d_tile.p, stride, P, 0, nullptr, nullptr, ctx->stream));
                HIP_TRY(ctx, cl_copy_sync(ctx, counts.data(), d_counts.p, groups * sizeof(uint32_t), hipMemcpyDeviceToHost));
                uint64_t block_sites = 0;   // counts -> their exclusive offsets
                for (uint32_t k = 0; k < groups; ++k) { const uint32_t c = counts[k]; counts[k] = (uint32_t)block_sites; block_sites += c; }
                if (block_sites) {
                    ScopedBuf<uint64_t> d_site_col;
                    ScopedBuf<char> d_site_rows;
                    if ((rc = d_site_col.alloc(ctx, block_sites)) || (rc = d_site_rows.alloc(ctx, P * block_sites))) return rc;
                    HIP_TRY(ctx, cl_copy_sync(ctx, d_offsets.p, counts.data(), groups * sizeof(uint32_t), hipMemcpyHostToDevice));
                    HIP_TRY(ctx, cl_launch_msa_sites(true, d_records.p, width, nullptr, d_offsets.p, c0, d_tile.p, stride, P, block_sites, d_site_col.p, d_site_rows.p,
                                                     ctx->stream));
                    const size_t before = site_col.size();
                    site_col.resize(before + block_sites);
                    site_pieces.emplace_back(P * block_sites);
                    piece_sites.push_back(block_sites);
                    HIP_TRY(ctx, hipMemcpyAsync(site_col.data() + before, d_site_col.p, block_sites * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
                    HIP_TRY(ctx, cl_copy_sync(ctx, site_pieces.back().data(), d_site_rows.p, P * block_sites, hipMemcpyDeviceToHost));
                }
            }
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the tile, the ranges and the records are reused by the next block
        }
    }
    if (want & kWantSites) {
        const uint64_t n_sites = site_col.size();
        out->n_sites = n_sites;
        if (!(out->site_col = alloc_array<uint64_t>(n_sites)) || !(out->site_rows = alloc_array<char>(P * n_sites))) return CL_ERR_OUT_OF_MEMORY;
        if (n_sites) memcpy(out->site_col, site_col.data(), n_sites * sizeof(uint64_t));
        uint64_t k0 = 0;   // the blocks' pieces side by side in every row
        for (size_t b = 0; b < site_pieces.size(); ++b) {
            for (uint64_t p = 0; p < P; ++p) memcpy(out->site_rows + p * n_sites + k0, site_pieces[b].data() + p * piece_sites[b], piece_sites[b]);
            k0 += piece_sites[b];
        }
    }
    guard.keep = true;
    return CL_OK;
}

}  // extern "C"
