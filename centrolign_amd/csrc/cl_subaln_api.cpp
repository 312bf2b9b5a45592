// cl_subaln_api.cpp — the two per-merge / per-bond text outputs of the CLI that are not the MSA itself:
//   cl_subalignment_text      -s: Core::emit_subalignment (src/core.cpp:424-472), one merge's block; the lines come from subaln_kernels.hip
//   cl_bond_alignment_cigar   --bond-prefix: Core::output_bond_alignment (include/centrolign/core.hpp:426-500), host code
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cl_internal.hpp"

namespace {

constexpr uint64_t kGap = ~(uint64_t)0;
// device text of one chunk of cl_subalignment_text when the caller gives no ceiling (as cl_induced_pairwise_cigars bounds its text)
constexpr uint64_t kDefaultChunkBytes = 256ull << 20;

// a growing malloc'ed text (handed to the caller as it is)
struct Text {
    char* p = nullptr;
    uint64_t n = 0, cap = 0;
    ~Text() { free(p); }
    char* reserve(uint64_t more) {
        if (n + more + 1 > cap) {
            uint64_t c = std::max<uint64_t>(cap * 2, n + more + 1);
            char* q = (char*)realloc(p, c);
            if (!q) return nullptr;
            p = q;
            cap = c;
        }
        return p + n;
    }
    bool add(const char* s, uint64_t len) {
        char* at = reserve(len);
        if (!at) return false;
        memcpy(at, s, len);
        n += len;
        return true;
    }
    char* release(uint64_t* len_out) {
        if (!reserve(0)) return nullptr;
        p[n] = '\0';
        if (len_out) *len_out = n;
        char* r = p;
        p = nullptr;
        return r;
    }
};

// one graph of the merge on the device: paths, labels, names and the step table; released where it goes out of scope
struct DevSide {
    ScopedBuf<uint64_t> path_off, name_off;
    ScopedBuf<uint32_t> path_nodes;
    ScopedBuf<uint8_t> label;
    ScopedBuf<char> names;
    ScopedBuf<unsigned long long> table;
    int load(cl_context* ctx, const cl_base_graph* g, const char* const* path_names, ClSubalnSide* view) {
        const uint64_t n_steps = g->path_off[g->n_paths];
        std::vector<uint64_t> noff(1, 0);
        std::string all;
        for (uint64_t p = 0; p < g->n_paths; ++p) { all += path_names[p]; noff.push_back(all.size()); }
        int rc;
        if ((rc = path_off.alloc(ctx, g->n_paths + 1)) || (rc = path_nodes.alloc(ctx, n_steps)) || (rc = label.alloc(ctx, g->n_nodes)) ||
            (rc = name_off.upload(ctx, noff)) || (rc = names.upload(ctx, all)) || (rc = table.alloc(ctx, g->n_nodes)))
            return rc;
        HIP_TRY(ctx, cl_copy_sync(ctx, path_off.p, g->path_off, (g->n_paths + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIP_TRY(ctx, cl_copy_sync(ctx, path_nodes.p, g->path_nodes, n_steps * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(ctx, cl_copy_sync(ctx, label.p, g->label, g->n_nodes, hipMemcpyHostToDevice));
        HIP_TRY(ctx, cl_launch_subaln_step_table(path_off.p, g->n_paths, path_nodes.p, n_steps, g->n_nodes, table.p, ctx->stream));
        *view = ClSubalnSide{table.p, label.p, g->n_nodes, names.p, name_off.p};
        return CL_OK;
    }
};

bool graph_ok(const cl_base_graph* g, const char* const* names) {
    if (!g || (g->n_paths && (!g->path_off || !g->path_nodes || !names)) || (g->n_nodes && !g->label)) return false;
    if (g->n_paths >= (1ull << 32)) return false;   // (path, step) share one 64-bit key
    for (uint64_t p = 0; p < g->n_paths; ++p)
        if (!names[p] || g->path_off[p + 1] < g->path_off[p] || g->path_off[p + 1] - g->path_off[p] > 0xFFFFFFFFull) return false;
    return true;
}

}  // namespace

extern "C" {

int cl_subalignment_text(cl_context* ctx, const cl_base_graph* g1, const char* const* path_names1, const char* const* set1, uint64_t n_set1,
                         const cl_base_graph* g2, const char* const* path_names2, const char* const* set2, uint64_t n_set2, const uint64_t* pairs,
                         uint64_t n_pairs, uint64_t chunk_bytes, char** text_out, uint64_t* len_out) {
    cl_bind_device(ctx);
    if (!ctx || !text_out || (n_pairs && !pairs) || (n_set1 && !set1) || (n_set2 && !set2) || !graph_ok(g1, path_names1) || !graph_ok(g2, path_names2)) {
        cl_set_error(ctx, "cl_subalignment_text: invalid argument");
        return CL_ERR_INVALID_ARGUMENT;
    }
    *text_out = nullptr;
    if (len_out) *len_out = 0;
    Text out;
    std::string head = "# sequence set 1\n";
    for (uint64_t i = 0; i < n_set1; ++i) { head += set1[i]; head += '\n'; }
    head += "# sequence set 2\n";
    for (uint64_t i = 0; i < n_set2; ++i) { head += set2[i]; head += '\n'; }
    head += "# alignment\n";
    if (!out.add(head.data(), head.size())) return CL_ERR_OUT_OF_MEMORY;
    if (n_pairs) {
        int rc;
        DevSide d1, d2;
        ClSubalnSide s1, s2;
        if ((rc = d1.load(ctx, g1, path_names1, &s1)) || (rc = d2.load(ctx, g2, path_names2, &s2))) return rc;
        // chunks of pairs whose text cannot exceed chunk_bytes: a side has at most max(5, name + 10 digits + 3) bytes
        uint64_t longest = 0;
        for (int s = 0; s < 2; ++s) {
            const cl_base_graph* g = s ? g2 : g1;
            for (uint64_t p = 0; p < g->n_paths; ++p) longest = std::max<uint64_t>(longest, strlen((s ? path_names2 : path_names1)[p]));
        }
        const uint64_t max_line = 2 * std::max<uint64_t>(5, longest + 13) + 2;
        const uint64_t per_chunk = std::min<uint64_t>(n_pairs, std::max<uint64_t>(1, (chunk_bytes ? chunk_bytes : kDefaultChunkBytes) / max_line));
        const uint64_t per_block = cl_subaln_pairs_per_block();
        ScopedBuf<uint64_t> d_pairs, d_off;   // (every return below gives the sixteen blocks back: cl_dev_free waits for the stream first)
        ScopedBuf<unsigned long long> d_bad;
        ScopedBuf<char> d_text;
        if ((rc = d_pairs.alloc(ctx, 2 * per_chunk)) || (rc = d_off.alloc(ctx, (per_chunk + per_block - 1) / per_block + 1)) || (rc = d_bad.alloc(ctx, 1)) ||
            (rc = d_text.alloc(ctx, per_chunk * max_line)))
            return rc;
        HIP_TRY(ctx, hipMemsetAsync(d_bad.p, 0xFF, sizeof(unsigned long long), ctx->stream));
        for (uint64_t c0 = 0; c0 < n_pairs; c0 += per_chunk) {
            const uint64_t n = std::min(per_chunk, n_pairs - c0), blocks = (n + per_block - 1) / per_block;
            HIP_TRY(ctx, hipMemcpyAsync(d_pairs.p, pairs + 2 * c0, 2 * n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, cl_launch_subaln_lengths(s1, s2, d_pairs.p, n, d_off.p, d_bad.p, ctx->stream));
            unsigned long long bad = 0;
            uint64_t bytes = 0;
            HIP_TRY(ctx, cl_copy_sync(ctx, &bad, d_bad.p, sizeof(bad), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, cl_copy_sync(ctx, &bytes, d_off.p + blocks, sizeof(bytes), hipMemcpyDeviceToHost));
            if (bad != ~0ull) {   // the first failing pair of the first failing chunk is the first failing pair
                const uint64_t k = c0 + bad, a = pairs[2 * k], b = pairs[2 * k + 1];
                const bool range = (a != kGap && a >= g1->n_nodes) || (b != kGap && b >= g2->n_nodes);
                cl_set_error(ctx, "subalignment pair %llu (%llu, %llu): %s", (unsigned long long)k, (unsigned long long)a, (unsigned long long)b,
                             range ? "a node id is out of range" : "a node is on no path");
                return CL_ERR_INVALID_ARGUMENT;
            }
            if (bytes > n * max_line) { cl_set_error(ctx, "cl_subalignment_text: %llu bytes exceed the chunk's bound", (unsigned long long)bytes); return CL_ERR_HIP; }
            HIP_TRY(ctx, cl_launch_subaln_write(s1, s2, d_pairs.p, n, d_off.p, d_text.p, ctx->stream));
            char* at = out.reserve(bytes);
            if (!at) return CL_ERR_OUT_OF_MEMORY;
            HIP_TRY(ctx, cl_copy_sync(ctx, at, d_text.p, bytes, hipMemcpyDeviceToHost));
            out.n += bytes;
        }
    }
    *text_out = out.release(len_out);
    return *text_out ? CL_OK : CL_ERR_OUT_OF_MEMORY;
}

int cl_bond_alignment_cigar(const cl_base_graph* g, uint64_t path, const uint64_t* pairs, uint64_t n_pairs, char** text_out, uint64_t* len_out) {
    if (!g || !text_out || (n_pairs && !pairs) || path >= g->n_paths) return CL_ERR_INVALID_ARGUMENT;
    *text_out = nullptr;
    if (len_out) *len_out = 0;
    const uint32_t* steps = g->path_nodes + g->path_off[path];
    const uint64_t len = g->path_off[path + 1] - g->path_off[path];
    // the boundaries: the first and last non-gap node on either side
    uint64_t first1 = kGap, first2 = kGap, last1 = kGap, last2 = kGap;
    for (uint64_t i = 0; i < n_pairs && (first1 == kGap || first2 == kGap); ++i) {
        if (first1 == kGap && pairs[2 * i] != kGap) first1 = pairs[2 * i];
        if (first2 == kGap && pairs[2 * i + 1] != kGap) first2 = pairs[2 * i + 1];
    }
    for (uint64_t i = n_pairs; i-- > 0 && (last1 == kGap || last2 == kGap);) {
        if (last1 == kGap && pairs[2 * i] != kGap) last1 = pairs[2 * i];
        if (last2 == kGap && pairs[2 * i + 1] != kGap) last2 = pairs[2 * i + 1];
    }
    Text out;
    if (first1 != kGap) {   // (no node on side 1: the reference writes the line end alone)
        std::vector<uint64_t> padded;
        for (uint64_t i = 0; i < len && steps[i] != first1; ++i) { padded.push_back(steps[i]); padded.push_back(kGap); }   // leading deletions
        for (uint64_t i = 0; i < len && steps[i] != first2; ++i) { padded.push_back(kGap); padded.push_back(steps[i]); }   // leading insertions
        padded.insert(padded.end(), pairs, pairs + 2 * n_pairs);
        const size_t lag = padded.size() / 2;
        for (uint64_t i = len; i-- > 0 && steps[i] != last2;) { padded.push_back(kGap); padded.push_back(steps[i]); }      // lagging insertions,
        for (uint64_t i = len; i-- > 0 && steps[i] != last1;) { padded.push_back(steps[i]); padded.push_back(kGap); }      // then deletions, backwards
        for (size_t a = lag, b = padded.size() / 2; a + 1 < b; ++a, --b) {                                                  // ... put in forward order
            std::swap(padded[2 * a], padded[2 * (b - 1)]);
            std::swap(padded[2 * a + 1], padded[2 * (b - 1) + 1]);
        }
        char* cigar = nullptr;
        uint64_t n = 0;
        const int rc = cl_explicit_cigar(g, g, padded.data(), padded.size() / 2, &cigar, &n);
        if (rc) return rc;
        const bool ok = out.add(cigar, n);
        free(cigar);
        if (!ok) return CL_ERR_OUT_OF_MEMORY;
    }
    if (!out.add("\n", 1)) return CL_ERR_OUT_OF_MEMORY;
    *text_out = out.release(len_out);
    return *text_out ? CL_OK : CL_ERR_OUT_OF_MEMORY;
}

}  // extern "C"
