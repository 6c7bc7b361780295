// Frame store on the device: the frame choice of the reference's loader for a batch of pairs of one data type, and the gather
// of the chosen frames into contiguous batch buffers (include/dcn_hip.h section 10).
//
//   select_kernel   ONE workgroup of kSelThreads; wavefront w takes pairs w, w + kSelWaves, ...  The object / scene / frame
//                   positions are computed redundantly by every lane of the wavefront (uniform values); the search for image
//                   b gives each lane one attempt, in chunks of 64: the first attempt that passes the pose test is the first
//                   set bit of the ballot.  Status bits are OR-ed in LDS and written once by thread 0.
//   gather_kernel   grid (chunks, slots x pairs): every work-item copies kGatherUnroll units of 16 bytes (1 byte when a plane
//                   size or a base pointer is not a multiple of 16) of one slot's RGB | depth | mask planes; the first
//                   workgroup of every even slot also writes the pair's camera row.
#include "dcn_common.h"

#if defined(DCN_HOSTEMU_BUILD)
static inline double dcn_dmul_rn(double a, double b) { return a * b; }
static inline double dcn_dadd_rn(double a, double b) { return a + b; }
#else
__device__ __forceinline__ double dcn_dmul_rn(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double dcn_dadd_rn(double a, double b) { return __dadd_rn(a, b); }
#endif

namespace {

constexpr int kSelThreads = 256;
constexpr int kSelWaves = kSelThreads / dcn::kWave;
constexpr int kMaxPairs = 65536;
constexpr int kMaxAttempts = 4096;
constexpr int kGatherThreads = 256;
constexpr int kGatherUnroll = 4;
constexpr int kCamFloats = DCN_SAMPLE_CAM_FLOATS;

enum DataType { WITHIN = 0, ACROSS = 1, DIFFERENT = 2, MULTI = 3, SYNTHETIC = 4 };
constexpr int kFatal = DCN_FRAME_BAD_INDEX | DCN_FRAME_NO_CANDIDATES;   // (a bad replay word reads as 0 and goes on)

struct SelArgs {
    dcn_frame_store st;
    const int64_t* seeds;          // [n] or null (replay)
    const int32_t* draws;          // [n][words] replay positions
    int32_t* frames;               // [n][DCN_FRAME_SLOTS]
    uint8_t* empty;                // [n]
    int32_t* scenes;               // [n][2]
    int32_t* objects;              // [n][2]
    int32_t* status;
    double threshold, angle_threshold;
    int n, type, attempts, words, use_angle;
};

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}

// Position in [0, len) of word k of pair p: the hash of (seed, k) scaled onto len, or the caller's replay position (outside
// [0, len): DCN_FRAME_BAD_DRAWS, read as 0).  len >= 1.
__device__ __forceinline__ int position(const SelArgs& a, int p, int k, int len, int& bad) {
    if (a.seeds) {
        const uint64_t s = (uint64_t)a.seeds[p];
        const uint32_t k0 = mix32((uint32_t)s ^ 0x5851F42DU);
        const uint32_t r = mix32(mix32((uint32_t)k ^ k0) ^ (mix32((uint32_t)(s >> 32) ^ k0) + 0x9E3779B9U));
        return (int)(((uint64_t)r * (uint32_t)len) >> 32);
    }
    const int v = a.draws[(size_t)p * a.words + k];
    if (v < 0 || v >= len) {
        bad |= DCN_FRAME_BAD_DRAWS;
        return 0;
    }
    return v;
}

// np.random.choice(len, 2, replace=False): two distinct positions (len >= 2); drawn: the second uniform over the other len - 1
__device__ __forceinline__ void two_positions(const SelArgs& a, int p, int k0, int k1, int len, int& i0, int& i1, int& bad) {
    if (a.seeds) {
        i0 = position(a, p, k0, len, bad);
        i1 = position(a, p, k1, len - 1, bad);
        if (i1 >= i0) ++i1;
        return;
    }
    i0 = position(a, p, k0, len, bad);
    i1 = position(a, p, k1, len, bad);
    if (i0 == i1) {
        bad |= DCN_FRAME_BAD_DRAWS;
        i1 = i0 + 1 < len ? i0 + 1 : 0;
    }
}

// Scene s's frames [first, first + count); false (DCN_FRAME_BAD_INDEX) when s or its range is outside the tables
__device__ __forceinline__ bool scene_range(const dcn_frame_store& st, int s, int64_t& first, int& count, int& bad) {
    if (s < 0 || s >= st.num_scenes) {
        bad |= DCN_FRAME_BAD_INDEX;
        return false;
    }
    first = st.scene_first_frame[s];
    const int64_t end = st.scene_first_frame[s + 1];
    if (first < 0 || end <= first || end > st.num_frames) {
        bad |= DCN_FRAME_BAD_INDEX;
        return false;
    }
    count = (int)(end - first);
    return true;
}

// get_img_idx_with_different_pose: the first of the attempts k_base .. k_base + attempts - 1 whose frame's pose passes the
// test against frame fa, or -1.  Called by the whole wavefront (uniform arguments).
__device__ int different_pose(const SelArgs& a, int p, int64_t first, int count, int64_t fa, int k_base, int& bad) {
    const int lane = threadIdx.x & (dcn::kWave - 1);
    const double* pa = a.st.poses + fa * 16;
    double Ra[9], ta[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Ra[3 * i + j] = pa[4 * i + j];
        ta[i] = pa[4 * i + 3];
    }
    for (int c0 = 0; c0 < a.attempts; c0 += dcn::kWave) {
        const int k = c0 + lane;
        int lane_bad = 0, pass = 0;
        int64_t cand = -1;
        if (k < a.attempts) {
            cand = first + position(a, p, k_base + k, count, lane_bad);
            const double* pb = a.st.poses + cand * 16;
            double sq = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double d = ta[i] - pb[4 * i + 3];
                sq = dcn_dadd_rn(sq, dcn_dmul_rn(d, d));
            }
            pass = sqrt(sq) > a.threshold;            // utils.compute_distance_between_poses: norm of the translation difference
            if (a.use_angle) {
                double tr = 0.0;                      // tr(R_a^T R_b) = sum_ij Ra_ij Rb_ij
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) tr = dcn_dadd_rn(tr, dcn_dmul_rn(Ra[3 * i + j], pb[4 * i + j]));
                double c = dcn_dmul_rn(tr - 1.0, 0.5);
                c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
                pass |= 2.0 * acos(c) > a.angle_threshold;
            }
        }
        const unsigned long long m = __ballot(pass);
        unsigned long long bm = __ballot(lane_bad != 0);
        if (m) {
            const int l = __builtin_ctzll(m);
            bm &= (2ull << l) - 1ull;                 // (attempts after the chosen one were never drawn by the reference)
            if (bm) bad |= DCN_FRAME_BAD_DRAWS;
            return (int)__shfl((int)cand, l);
        }
        if (bm) bad |= DCN_FRAME_BAD_DRAWS;
    }
    return -1;
}

// A uniform scene of object o (random.choice over its list); -1 with DCN_FRAME_NO_CANDIDATES / BAD_INDEX
__device__ __forceinline__ int object_scene(const SelArgs& a, int p, int o, int k, int& bad) {
    const int lo = a.st.object_scene_offsets[o], hi = a.st.object_scene_offsets[o + 1];
    if (hi <= lo) {
        bad |= DCN_FRAME_NO_CANDIDATES;
        return -1;
    }
    return a.st.object_scenes[lo + position(a, p, k, hi - lo, bad)];
}

// One pair, the whole wavefront (every value below is uniform across its lanes)
__device__ void select_pair(const SelArgs& a, int p, int& bad) {
    const int lane = threadIdx.x & (dcn::kWave - 1);
    int f[DCN_FRAME_SLOTS] = {-1, -1, -1, -1};
    int sc[2] = {-1, -1}, ob[2] = {-1, -1};
    int empty = 1;
    const int O = a.st.num_objects;
    int pair_bad = 0;
    int64_t first_a = 0, first_b = 0;
    int cnt_a = 0, cnt_b = 0;
    if (a.type == WITHIN || a.type == MULTI) {
        if (a.type == MULTI) {
            if (a.st.num_multi < 1) pair_bad |= DCN_FRAME_NO_CANDIDATES;
            else sc[0] = a.st.multi_scenes[position(a, p, DCN_FRAME_DRAW_SCENE_A, a.st.num_multi, pair_bad)];
        } else if (O < 1) {
            pair_bad |= DCN_FRAME_NO_CANDIDATES;
        } else {
            ob[0] = ob[1] = position(a, p, DCN_FRAME_DRAW_OBJECT_A, O, pair_bad);
            sc[0] = object_scene(a, p, ob[0], DCN_FRAME_DRAW_SCENE_A, pair_bad);
        }
        sc[1] = sc[0];
        if (!(pair_bad & kFatal) && scene_range(a.st, sc[0], first_a, cnt_a, pair_bad)) {
            f[0] = (int)(first_a + position(a, p, DCN_FRAME_DRAW_FRAME_A, cnt_a, pair_bad));
            f[1] = different_pose(a, p, first_a, cnt_a, f[0], DCN_FRAME_DRAW_HEADER, pair_bad);
            empty = f[1] < 0;
        }
    } else if (a.type == ACROSS) {
        if (O < 1) {
            pair_bad |= DCN_FRAME_NO_CANDIDATES;
        } else {
            ob[0] = ob[1] = position(a, p, DCN_FRAME_DRAW_OBJECT_A, O, pair_bad);
            const int lo = a.st.object_scene_offsets[ob[0]], len = a.st.object_scene_offsets[ob[0] + 1] - lo;
            if (len < 2) {
                pair_bad |= DCN_FRAME_NO_CANDIDATES;     // get_different_scene_for_object's ValueError
            } else {
                sc[0] = a.st.object_scenes[lo + position(a, p, DCN_FRAME_DRAW_SCENE_A, len, pair_bad)];
                int i0, i1;
                two_positions(a, p, DCN_FRAME_DRAW_SCENE_B, DCN_FRAME_DRAW_SCENE_B2, len, i0, i1, pair_bad);
                sc[1] = a.st.object_scenes[lo + i0] != sc[0] ? a.st.object_scenes[lo + i0] : a.st.object_scenes[lo + i1];
            }
        }
    } else {   // DIFFERENT, SYNTHETIC
        if (O < 2) {
            pair_bad |= DCN_FRAME_NO_CANDIDATES;     // get_two_different_object_ids' ValueError
        } else {
            two_positions(a, p, DCN_FRAME_DRAW_OBJECT_A, DCN_FRAME_DRAW_OBJECT_B, O, ob[0], ob[1], pair_bad);
            sc[0] = object_scene(a, p, ob[0], DCN_FRAME_DRAW_SCENE_A, pair_bad);
            if (!(pair_bad & kFatal)) sc[1] = object_scene(a, p, ob[1], DCN_FRAME_DRAW_SCENE_B, pair_bad);
        }
    }
    if (a.type == ACROSS || a.type == DIFFERENT || a.type == SYNTHETIC) {
        if (!(pair_bad & kFatal) && scene_range(a.st, sc[0], first_a, cnt_a, pair_bad) &&
            scene_range(a.st, sc[1], first_b, cnt_b, pair_bad)) {
            f[0] = (int)(first_a + position(a, p, DCN_FRAME_DRAW_FRAME_A, cnt_a, pair_bad));
            if (a.type != SYNTHETIC) {
                f[1] = (int)(first_b + position(a, p, DCN_FRAME_DRAW_FRAME_B, cnt_b, pair_bad));
                empty = 0;
            } else {
                f[1] = different_pose(a, p, first_a, cnt_a, f[0], DCN_FRAME_DRAW_HEADER, pair_bad);
                f[2] = (int)(first_b + position(a, p, DCN_FRAME_DRAW_FRAME_B, cnt_b, pair_bad));
                f[3] = different_pose(a, p, first_b, cnt_b, f[2], DCN_FRAME_DRAW_HEADER + a.attempts, pair_bad);
                empty = f[1] < 0 || f[3] < 0;
            }
        }
    }
    if (f[0] < 0) {
        empty = 1;                                   // no eligible scene / bad tables: every slot -1 (the gather zero-fills)
    } else if (empty) {                              // return_empty_data(image_a, image_a): a missing image b is image a
        if (f[1] < 0) f[1] = f[0];
        if (a.type == SYNTHETIC && f[3] < 0) f[3] = f[2];
    }
    bad |= pair_bad;
    // (lane-selected values through selects, not a dynamically indexed private array)
    if (lane < DCN_FRAME_SLOTS)
        a.frames[(size_t)p * DCN_FRAME_SLOTS + lane] = lane == 0 ? f[0] : lane == 1 ? f[1] : lane == 2 ? f[2] : f[3];
    if (lane < 2) {
        a.scenes[(size_t)p * 2 + lane] = lane == 0 ? sc[0] : sc[1];
        a.objects[(size_t)p * 2 + lane] = lane == 0 ? ob[0] : ob[1];
    }
    if (lane == 0) a.empty[p] = (uint8_t)empty;
}

__global__ void __launch_bounds__(kSelThreads) select_kernel(SelArgs a) {
    __shared__ int32_t bad_s[kSelWaves];
    const int wv = threadIdx.x / dcn::kWave;
    int bad = 0;
    for (int p = wv; p < a.n; p += kSelWaves) select_pair(a, p, bad);
    if ((threadIdx.x & (dcn::kWave - 1)) == 0) bad_s[wv] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int i = 0; i < kSelWaves; ++i) s |= bad_s[i];
        a.status[0] = s;
    }
}

struct GatherArgs {
    dcn_frame_store st;
    const int32_t* frames;
    const uint8_t* empty;
    uint8_t* rgb;
    uint8_t* depth;                // uint16 planes, copied as bytes
    uint8_t* mask;
    float* cams;
    int32_t* status;
    int64_t hw;
    int64_t units_rgb, units_depth, units_mask;   // per slot, in units of the copy width
    int n, k;
};

// The rows of section 9's cams for slots (2j, 2j+1) of pair p: thread t < kCamFloats writes entry t
__device__ void camera_row(const GatherArgs& g, int p, int j) {
    const int t = threadIdx.x;
    if (t >= kCamFloats) return;
    const int64_t fa = g.frames[(size_t)p * DCN_FRAME_SLOTS + 2 * j], fb = g.frames[(size_t)p * DCN_FRAME_SLOTS + 2 * j + 1];
    float* row = g.cams + ((size_t)j * g.n + p) * kCamFloats;
    if (fa < 0 || fa >= g.st.num_frames || fb < 0 || fb >= g.st.num_frames) {
        row[t] = 0.f;
        return;
    }
    if (t < 2 * 9) {
        int lo = 0, hi = g.st.num_scenes - 1;                 // the scene of frame a: last s with scene_first_frame[s] <= fa
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (g.st.scene_first_frame[mid] <= fa) lo = mid;
            else hi = mid - 1;
        }
        row[t] = g.st.scene_cams[(size_t)lo * DCN_FRAME_CAM_FLOATS + t];
    } else if (t < 2 * 9 + 16) {
        row[t] = (float)g.st.poses[fa * 16 + (t - 18)];
    } else {
        const int e = t - 34, i = e >> 2, c = e & 3;
        const double* pb = g.st.poses + fb * 16;
        double v;
        if (i == 3) {
            v = c == 3 ? 1.0 : 0.0;
        } else if (c < 3) {
            v = pb[4 * c + i];                                  // (R^T)_ic
        } else {                                                // -(R^T t)_i, summed left to right (numpy's dot order)
            double s = dcn_dmul_rn(pb[i], pb[3]);
            s = dcn_dadd_rn(s, dcn_dmul_rn(pb[4 + i], pb[7]));
            s = dcn_dadd_rn(s, dcn_dmul_rn(pb[8 + i], pb[11]));
            v = -s;
        }
        row[t] = (float)v;
    }
}

template <class V>
__global__ void __launch_bounds__(kGatherThreads) gather_kernel(GatherArgs g) {
    const int slot = blockIdx.y / g.n, p = blockIdx.y - slot * g.n;
    const int64_t f = g.frames[(size_t)p * DCN_FRAME_SLOTS + slot];
    const bool valid = f >= 0 && f < g.st.num_frames;
    const bool zero_depth = !valid || (g.empty && g.empty[p]);
    if (blockIdx.x == 0 && threadIdx.x == 0 && !valid) atomicOr(g.status, DCN_FRAME_BAD_INDEX);
    if (blockIdx.x == 0 && g.cams && (slot & 1) == 0) camera_row(g, p, slot >> 1);
    const int64_t total = g.units_rgb + g.units_depth + g.units_mask;
    const size_t dst_slot = (size_t)slot * g.n + p;
    const int64_t u0 = ((int64_t)blockIdx.x * kGatherUnroll) * kGatherThreads + threadIdx.x;
    V v[kGatherUnroll];
    V* dst[kGatherUnroll];
#pragma unroll
    for (int r = 0; r < kGatherUnroll; ++r) {        // every load of the work-item issued before its first store
        int64_t u = u0 + (int64_t)r * kGatherThreads;
        dst[r] = nullptr;
        v[r] = V{};
        if (u >= total) continue;
        const V* src;
        bool zero = !valid;
        if (u < g.units_rgb) {
            src = reinterpret_cast<const V*>(g.st.rgb) + (valid ? f : 0) * g.units_rgb + u;
            dst[r] = reinterpret_cast<V*>(g.rgb) + dst_slot * g.units_rgb + u;
        } else if ((u -= g.units_rgb) < g.units_depth) {
            src = reinterpret_cast<const V*>(g.st.depth) + (valid ? f : 0) * g.units_depth + u;
            dst[r] = reinterpret_cast<V*>(g.depth) + dst_slot * g.units_depth + u;
            zero = zero_depth;
        } else {
            u -= g.units_depth;
            src = reinterpret_cast<const V*>(g.st.mask) + (valid ? f : 0) * g.units_mask + u;
            dst[r] = reinterpret_cast<V*>(g.mask) + dst_slot * g.units_mask + u;
        }
        if (!zero) v[r] = *src;
    }
#pragma unroll
    for (int r = 0; r < kGatherUnroll; ++r)
        if (dst[r]) *dst[r] = v[r];
}

bool store_ok(const dcn_frame_store* s) {
    return s && s->num_frames >= 1 && s->num_frames <= (int64_t)INT32_MAX && s->num_scenes >= 1 && s->num_objects >= 0 &&
           s->num_multi >= 0 && s->h >= 1 && s->w >= 1 && s->scene_first_frame && s->scene_object && s->poses &&
           s->scene_cams && s->object_scene_offsets && (s->num_objects == 0 || s->object_scenes) &&
           (s->num_multi == 0 || s->multi_scenes);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int dcn_select_frames(int n, int data_type, const dcn_frame_store* store, int num_attempts, double threshold,
                                 double angle_threshold, const int64_t* seeds, const int32_t* draws, int32_t* frames,
                                 uint8_t* empty, int32_t* scenes, int32_t* objects, int32_t* status, void* stream) {
    if (n < 1 || n > kMaxPairs || data_type < WITHIN || data_type > SYNTHETIC || !store_ok(store) || num_attempts < 1 ||
        num_attempts > kMaxAttempts || (!seeds && !draws) || !frames || !empty || !scenes || !objects || !status ||
        !(threshold == threshold) || !(angle_threshold == angle_threshold))
        return DCN_E_INVALID;
    SelArgs a;
    a.st = *store;
    a.seeds = seeds;
    a.draws = draws;
    a.frames = frames;
    a.empty = empty;
    a.scenes = scenes;
    a.objects = objects;
    a.status = status;
    a.threshold = threshold;
    a.angle_threshold = angle_threshold;
    a.use_angle = angle_threshold < 2.0 * 3.14159265358979323846;   // the angle is at most 2 pi: the clause never passes
    a.n = n;
    a.type = data_type;
    a.attempts = num_attempts;
    a.words = DCN_FRAME_DRAW_HEADER + 2 * num_attempts;
    hipLaunchKernelGGL(select_kernel, dim3(1), dim3(kSelThreads), 0, (hipStream_t)stream, a);
    return dcn::check_launch();
}

extern "C" int dcn_gather_frames(int n, int frames_per_pair, const dcn_frame_store* store, const int32_t* frames,
                                 const uint8_t* empty, uint8_t* rgb, uint16_t* depth, uint8_t* mask, float* cams,
                                 int32_t* status, void* stream) {
    if (n < 1 || n > kMaxPairs || (frames_per_pair != 2 && frames_per_pair != 4) || !store_ok(store) || !frames || !status ||
        (rgb && !store->rgb) || (depth && !store->depth) || (mask && !store->mask))
        return DCN_E_INVALID;
    GatherArgs g;
    g.st = *store;
    g.frames = frames;
    g.empty = empty;
    g.rgb = rgb;
    g.depth = reinterpret_cast<uint8_t*>(depth);
    g.mask = mask;
    g.cams = cams;
    g.status = status;
    g.hw = (int64_t)store->h * store->w;
    g.n = n;
    g.k = frames_per_pair;
    const bool vec = g.hw % 16 == 0 && aligned16(rgb) && aligned16(depth) && aligned16(mask) && aligned16(store->rgb) &&
                     aligned16(store->depth) && aligned16(store->mask);
    const int64_t unit = vec ? 16 : 1;
    g.units_rgb = rgb ? 3 * g.hw / unit : 0;
    g.units_depth = depth ? 2 * g.hw / unit : 0;
    g.units_mask = mask ? g.hw / unit : 0;
    const int64_t per_block = (int64_t)kGatherThreads * kGatherUnroll;
    int64_t blocks = dcn::ceil_div64(g.units_rgb + g.units_depth + g.units_mask, per_block);
    if (blocks < 1) blocks = 1;                                   // (the camera rows)
    if (blocks > 65535 || (int64_t)n * frames_per_pair > 65535) return DCN_E_INVALID;
    const dim3 grid((unsigned)blocks, (unsigned)(n * frames_per_pair));
    if (vec) hipLaunchKernelGGL(gather_kernel<uint4>, grid, dim3(kGatherThreads), 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(gather_kernel<uint8_t>, grid, dim3(kGatherThreads), 0, (hipStream_t)stream, g);
    return dcn::check_launch();
}
