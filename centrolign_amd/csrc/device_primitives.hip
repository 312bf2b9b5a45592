// device_primitives.hip — the C ABI over the device primitives that the suffix array (match_kernels.hip), the guide tree's k-mer spectra (tree_kernels.hip),
// the far pass's static orders (chain_far.hip) and the traceback's value index (chain_sort.hip) stand on: cl_radix.h's stable radix sort and inclusive
// prefix sum, and the value index itself on both of its routes.  Host arrays in, host arrays out — like cl_suffix_array_lcp, "the device half" on its own,
// so that a test can hold every tile count, digit width and key encoding against an exact reference instead of meeting them through a whole feature.
// Nothing here is on a hot path: each call allocates, uploads, runs on the context's stream, downloads and releases.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chain_dp.hpp"   // cl_chain_sort_values, clchain::value_index_host
#include "cl_internal.hpp"
#include "cl_radix.h"

namespace {

template <class K>
int sort_pairs_on_device(cl_context* ctx, const K* keys_in, const uint32_t* vals_in, size_t n, unsigned begin_bit, unsigned end_bit, K* keys_out, uint32_t* vals_out) {
    hipStream_t s = ctx->stream;
    ScopedBuf<K> k_in, k_out;
    ScopedBuf<uint32_t> v_in, v_out;
    ScopedBuf<char> temp;
    const size_t temp_bytes = clradix::sort_temp_bytes<K>(n);
    int rc;
    if ((rc = k_in.alloc(ctx, n)) || (rc = k_out.alloc(ctx, n)) || (rc = v_in.alloc(ctx, n)) || (rc = v_out.alloc(ctx, n)) || (rc = temp.alloc(ctx, temp_bytes))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(k_in.p, keys_in, n * sizeof(K), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(v_in.p, vals_in, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, clradix::sort_pairs<K>(temp.p, temp_bytes, k_in.p, k_out.p, v_in.p, v_out.p, n, begin_bit, end_bit, s));
    HIP_TRY(ctx, hipMemcpyAsync(keys_out, k_out.p, n * sizeof(K), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(vals_out, v_out.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return CL_OK;
}

int refuse(cl_context* ctx, const char* entry, const char* what) {
    cl_set_error(ctx, "%s: %s", entry, what);
    return CL_ERR_INVALID_ARGUMENT;
}

}  // namespace

int cl_device_sort_pairs(cl_context* ctx, int key_bytes, const void* keys_in, const uint32_t* vals_in, uint64_t n, uint32_t begin_bit, uint32_t end_bit,
                         void* keys_out, uint32_t* vals_out) {
    cl_bind_device(ctx);
    if (!ctx) return refuse(ctx, "cl_device_sort_pairs", "null context");
    if (key_bytes != 4 && key_bytes != 8) return refuse(ctx, "cl_device_sort_pairs", "key_bytes must be 4 or 8");
    if (end_bit <= begin_bit) return refuse(ctx, "cl_device_sort_pairs", "end_bit must be above begin_bit");
    if (end_bit > 8u * (uint32_t)key_bytes) return refuse(ctx, "cl_device_sort_pairs", "end_bit beyond the key's width");
    if (n >= (1ull << 32)) return refuse(ctx, "cl_device_sort_pairs", "n must be below 2^32");
    if (n == 0) return CL_OK;
    if (!keys_in || !vals_in || !keys_out || !vals_out) return refuse(ctx, "cl_device_sort_pairs", "null array");
    if (key_bytes == 4)
        return sort_pairs_on_device<uint32_t>(ctx, static_cast<const uint32_t*>(keys_in), vals_in, (size_t)n, begin_bit, end_bit, static_cast<uint32_t*>(keys_out), vals_out);
    return sort_pairs_on_device<uint64_t>(ctx, static_cast<const uint64_t*>(keys_in), vals_in, (size_t)n, begin_bit, end_bit, static_cast<uint64_t*>(keys_out), vals_out);
}

int cl_device_inclusive_sum(cl_context* ctx, const uint32_t* in, uint64_t n, uint32_t* out) {
    cl_bind_device(ctx);
    if (!ctx) return refuse(ctx, "cl_device_inclusive_sum", "null context");
    if (n >= (1ull << 32)) return refuse(ctx, "cl_device_inclusive_sum", "n must be below 2^32");
    if (n == 0) return CL_OK;
    if (!in || !out) return refuse(ctx, "cl_device_inclusive_sum", "null array");
    hipStream_t s = ctx->stream;
    ScopedBuf<uint32_t> d_in, d_out;
    ScopedBuf<char> temp;
    const size_t temp_bytes = clradix::scan_temp_bytes((size_t)n);
    int rc;
    if ((rc = d_in.alloc(ctx, (size_t)n)) || (rc = d_out.alloc(ctx, (size_t)n)) || (rc = temp.alloc(ctx, temp_bytes))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_in.p, in, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, clradix::inclusive_sum(temp.p, temp_bytes, d_in.p, d_out.p, (size_t)n, s));
    HIP_TRY(ctx, hipMemcpyAsync(out, d_out.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return CL_OK;
}

// what ChainTrace::prepare_index and ChainTrace::value_index do for a DP that is not packed: the size of the scratch by a first call, the index by a second
int cl_chain_value_index(cl_context* ctx, const float* values, uint32_t n, int32_t* keys_out, uint32_t* recs_out) {
    cl_bind_device(ctx);
    if (!ctx) return refuse(ctx, "cl_chain_value_index", "null context");
    if (n == 0) return CL_OK;
    if (!values || !keys_out || !recs_out) return refuse(ctx, "cl_chain_value_index", "null array");
    hipStream_t s = ctx->stream;
    ScopedBuf<float> val;
    ScopedBuf<int> k_in, k_out;
    ScopedBuf<uint32_t> i_in, i_out;
    ScopedBuf<char> temp;
    int rc;
    if ((rc = val.alloc(ctx, n)) || (rc = k_in.alloc(ctx, n)) || (rc = k_out.alloc(ctx, n)) || (rc = i_in.alloc(ctx, n)) || (rc = i_out.alloc(ctx, n))) return rc;
    size_t temp_bytes = 0;
    HIP_TRY(ctx, cl_chain_sort_values(nullptr, n, k_in.p, i_in.p, k_out.p, i_out.p, nullptr, &temp_bytes, s));
    if ((rc = temp.alloc(ctx, temp_bytes))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(val.p, values, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, cl_chain_sort_values(val.p, n, k_in.p, i_in.p, k_out.p, i_out.p, temp.p, &temp_bytes, s));
    HIP_TRY(ctx, hipMemcpyAsync(keys_out, k_out.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(recs_out, i_out.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return CL_OK;
}

int cl_chain_value_index_host(const float* values, uint32_t n, int32_t* keys_out, uint32_t* recs_out) {
    if (n == 0) return CL_OK;
    if (!values || !keys_out || !recs_out) return refuse(nullptr, "cl_chain_value_index_host", "null array");
    clchain::value_index_host(values, n, keys_out, recs_out);
    return CL_OK;
}
