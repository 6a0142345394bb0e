// gather.hip -- stito_gather_crops: the evaluate-time inputs of a ragged multi-pair batch, cut out of one packed buffer.
//
// A pure copy (4 bytes read + 4 written per sample, HBM-bound): one workgroup row per (slot, channel), 16 bytes per lane where the
// row's source address allows it, one dword per lane (still consecutive across the wave) where it does not -- an odd crop start, a
// length that is not a multiple of four.  Nothing but plain vector loads and stores.
#include "common.h"

namespace stito {

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_VEC_PER_THREAD = 4;   // 16 KB of a row per workgroup on the vector path

__global__ __launch_bounds__(GATHER_THREADS) void k_gather_crops(const float *__restrict__ packed, int64_t packed_floats,
                                                                 const int64_t *__restrict__ offset, const int64_t *__restrict__ length,
                                                                 const int64_t *__restrict__ start, int n_pairs,
                                                                 const int32_t *__restrict__ slots, int channels, int64_t crop_len,
                                                                 float *__restrict__ out) {
    const int row = blockIdx.y;               // slot * channels + channel
    const int slot = row / channels, c = row - slot * channels;
    const int pair = slots[slot];
    float *dst = out + (int64_t)row * crop_len;
    // a slot that names no pair, or a pair whose (offset, length) does not lie inside the packed buffer, reads nothing: zeros
    int64_t len = 0, st = 0, src_off = 0;
    if (pair >= 0 && pair < n_pairs) {
        len = length[pair];
        st = start[pair];
        src_off = offset[pair];
        if (len < 0 || src_off < 0 || src_off > packed_floats || len > (packed_floats - src_off) / channels) len = 0;
        src_off += (int64_t)c * len;
    }
    const float *src = packed + src_off;      // sample j of this channel at src[j], 0 <= j < len
    const int64_t span = (int64_t)GATHER_THREADS * GATHER_VEC_PER_THREAD * 4;     // samples per workgroup
    const int64_t i0 = (int64_t)blockIdx.x * span;
    const int64_t i1 = i0 + span < crop_len ? i0 + span : crop_len;
    const bool vec = crop_len % 4 == 0 && ((uintptr_t)dst & 15) == 0 && (((uintptr_t)src + (uintptr_t)st * 4) & 15) == 0;   // uniform per workgroup
    if (vec) {
        for (int64_t i = i0 + (int64_t)threadIdx.x * 4; i < i1; i += GATHER_THREADS * 4) {
            const int64_t j = st + i;
            float4 v;
            if (j >= 0 && j + 3 < len) {
                v = *reinterpret_cast<const float4 *>(src + j);
            } else {
                v.x = (j >= 0 && j < len) ? src[j] : 0.0f;
                v.y = (j + 1 >= 0 && j + 1 < len) ? src[j + 1] : 0.0f;
                v.z = (j + 2 >= 0 && j + 2 < len) ? src[j + 2] : 0.0f;
                v.w = (j + 3 >= 0 && j + 3 < len) ? src[j + 3] : 0.0f;
            }
            *reinterpret_cast<float4 *>(dst + i) = v;
        }
    } else {
        for (int64_t i = i0 + threadIdx.x; i < i1; i += GATHER_THREADS) {
            const int64_t j = st + i;
            dst[i] = (j >= 0 && j < len) ? src[j] : 0.0f;
        }
    }
}

}  // namespace stito

extern "C" int stito_gather_crops(const float *packed_dev, int64_t packed_floats, const int64_t *offset_dev, const int64_t *length_dev,
                                  const int64_t *start_dev, int n_pairs, const int32_t *slots_dev, int n_slots, int channels,
                                  int64_t crop_len, float *out_dev, void *stream) {
    using namespace stito;
    STITO_REQUIRE(packed_dev && offset_dev && length_dev && start_dev && slots_dev && out_dev, STITO_E_INVALID,
                  "stito_gather_crops: null pointer");
    STITO_REQUIRE(packed_floats > 0 && n_pairs > 0 && n_slots > 0 && crop_len > 0, STITO_E_INVALID,
                  "stito_gather_crops: empty input (packed_floats %lld, n_pairs %d, n_slots %d, crop_len %lld)", (long long)packed_floats,
                  n_pairs, n_slots, (long long)crop_len);
    STITO_REQUIRE(channels == 1 || channels == 2, STITO_E_INVALID, "stito_gather_crops: %d channels (1 or 2)", channels);
    STITO_REQUIRE(((uintptr_t)packed_dev & 3) == 0 && ((uintptr_t)out_dev & 3) == 0, STITO_E_INVALID,
                  "stito_gather_crops: buffers must be float aligned");
    const int64_t span = (int64_t)GATHER_THREADS * GATHER_VEC_PER_THREAD * 4;
    const int64_t gx = (crop_len + span - 1) / span;
    const int64_t gy = (int64_t)n_slots * channels;
    STITO_REQUIRE(gx <= 0x7fffffff && gy <= 65535, STITO_E_INVALID, "stito_gather_crops: %d slots x %d channels x %lld samples exceed the grid",
                  n_slots, channels, (long long)crop_len);
    hipLaunchKernelGGL(k_gather_crops, dim3((unsigned)gx, (unsigned)gy), dim3(GATHER_THREADS), 0, (hipStream_t)stream, packed_dev,
                       packed_floats, offset_dev, length_dev, start_dev, n_pairs, slots_dev, channels, crop_len, out_dev);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}
