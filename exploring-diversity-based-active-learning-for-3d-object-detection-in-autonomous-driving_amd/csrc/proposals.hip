// TransFusion query initialisation on device (bevfusion/mmdet3d/models/heads/bbox/transfusion.py:236-275): from the dense
// class heat map of a BEV grid pick the num_proposals best (class, cell) pairs among the local maxima and build the
// decoder's initial queries.
//   reference:  heatmap = sigmoid(dense_heatmap); local_max = max_pool2d(heatmap, k, stride 1) on the interior (the k//2-wide
//               frame never proposes); classes of small objects (nuScenes 8, 9; Waymo 1, 2) keep every cell;
//               heatmap *= (heatmap == local_max); top = heatmap.view(B, -1).argsort(descending)[:, :P];
//               class = top // HW, cell = top % HW; query_feat = lidar_feat[cell] + class_encoding(one_hot(class));
//               query_pos = bev_pos[cell]; query_heatmap_score = heatmap[:, :, cell].
// Here: (1) one thread per cell evaluates the sigmoid of its C logits and of the ring around it and writes the masked scores
// as order-preserving 32-bit keys [B][C * HW] (a non-negative float's bits sort like the float); (2) one workgroup per
// sample selects and sorts the P largest keys with the pieces and the tie rule of al3d_select.h (flat index = class * HW +
// cell; the reference's argsort leaves ties unspecified) and writes
// class, cell, the C masked scores of each winning cell, the query position and the query feature row (gathered token row +
// the class-encoding column + bias).  No library kernel between the heat-map convolution and the decoder.
// Fewer positive masked scores than proposals: the remaining winners are zero-score cells in ascending flat index, so the P
// winners are always distinct.
// NaN logits: the score of such a cell is NaN, and as a key its bits lie above every finite score's, so where the cell may
// propose (interior, or a free class) it is taken FIRST, as torch's descending argsort puts it; on the frame of another class
// it is masked to 0 like any score (the reference's heatmap * 0 keeps it NaN there).  A NaN never suppresses a neighbour
// (the reference's max_pool2d would: `neighbour > score` is false here).  Class, cell, positions and features stay in
// range and distinct; only the NaN cells' own masked scores are NaN.
#include "al3d_common.h"
#include "al3d_select.h"

#define TP_THREADS 1024
#define TP_MAXP 256

// logits [B][H][W][C] (channels-last) -> keys [B][C][H*W] (bits of the masked sigmoid score; 0 = not a local maximum)
__global__ __launch_bounds__(256) void tp_peak_kernel(const float* __restrict__ logits, int B, int H, int W, int C, int k,
                                                      unsigned free_mask, unsigned* __restrict__ keys)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * H * W) return;
    const int x = (int)(t % W), y = (int)((t / W) % H), b = (int)(t / ((int64_t)W * H));
    const int r = k / 2;
    const bool interior = y >= r && y < H - r && x >= r && x < W - r;
    const float* row = logits + ((int64_t)b * H * W) * C;
    for (int c = 0; c < C; ++c) {
        const float s = al3d_sigmoid(row[((int64_t)y * W + x) * C + c]);
        bool peak = r == 0 || ((free_mask >> c) & 1u);
        if (!peak && interior) {
            peak = true;
            for (int dy = -r; dy <= r && peak; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    if (!dy && !dx) continue;
                    if (al3d_sigmoid(row[((int64_t)(y + dy) * W + (x + dx)) * C + c]) > s) { peak = false; break; }
                }
        }
        keys[((int64_t)b * C + c) * H * W + (int64_t)y * W + x] = peak ? __float_as_uint(s) : 0u;
    }
}

__global__ __launch_bounds__(TP_THREADS) void tp_select_kernel(const unsigned* __restrict__ keys, int HW, int C, int P,
                                                               const float* __restrict__ tokens, int hidden,
                                                               const float* __restrict__ bev_pos,
                                                               const float* __restrict__ class_cols,     // [C][hidden]
                                                               const float* __restrict__ class_bias,     // [hidden]
                                                               int64_t* __restrict__ top_class, int64_t* __restrict__ top_cell,
                                                               float* __restrict__ qscore, float* __restrict__ qfeat,
                                                               float* __restrict__ qpos)
{
    __shared__ SelScratch<TP_THREADS> sel;
    __shared__ unsigned long long s_sel[TP_MAXP];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t N = (int64_t)C * HW;
    const unsigned* kb = keys + (int64_t)b * N;
    for (int i = tid; i < TP_MAXP; i += TP_THREADS) s_sel[i] = 0ull;          // padding sorts last (key 0, index "infinity")
    // ---- the P largest keys (N >= P: exactly P words), then sorted: key descending, index ascending
    unsigned T, need;
    blk_radix_threshold<TP_THREADS>(kb, (int)N, (unsigned)P, sel, T, need);     // barriers inside: the padding is visible
    blk_collect_topk<TP_THREADS>(kb, (int)N, T, need, 0u, s_sel, TP_MAXP, sel);
    blk_sort_desc_u64<TP_THREADS>(s_sel, TP_MAXP);
    // ---- outputs
    for (int p = tid; p < P; p += TP_THREADS) {
        const unsigned idx = sel_word_index(s_sel[p]);
        top_class[(int64_t)b * P + p] = idx / HW;
        top_cell[(int64_t)b * P + p] = idx % HW;
    }
    for (int e = tid; e < P * C; e += TP_THREADS) {
        const int c = e / P, p = e % P;
        const unsigned idx = sel_word_index(s_sel[p]);
        qscore[((int64_t)b * C + c) * P + p] = __uint_as_float(kb[(int64_t)c * HW + idx % HW]);
    }
    for (int e = tid; e < P * 2; e += TP_THREADS) {
        const int p = e >> 1;
        const unsigned idx = sel_word_index(s_sel[p]);
        qpos[((int64_t)b * P + p) * 2 + (e & 1)] = bev_pos[(int64_t)(idx % HW) * 2 + (e & 1)];
    }
    for (int e = tid; e < P * hidden; e += TP_THREADS) {
        const int p = e / hidden, h = e % hidden;
        const unsigned idx = sel_word_index(s_sel[p]);
        const int cls = idx / HW, cell = idx % HW;
        // key_rows[cell] + class_encoding.weight[:, cls] + bias, in that order (the reference adds the Conv1d output)
        qfeat[((int64_t)b * P + p) * hidden + h] =
            tokens[((int64_t)b * HW + cell) * hidden + h] + (class_cols[(int64_t)cls * hidden + h] + class_bias[h]);
    }
}

extern "C" int64_t al3d_tf_proposals_workspace_bytes(int B, int H, int W, int C)
{
    return al3d_align((int64_t)(B > 0 ? B : 1) * H * W * C * 4, 256);
}

extern "C" int al3d_tf_proposals_f32(const float* heat_logits, int B, int H, int W, int C, int nms_kernel, unsigned free_class_mask,
                                     int P, const float* tokens, int hidden, const float* bev_pos, const float* class_cols,
                                     const float* class_bias, void* workspace, int64_t* top_class, int64_t* top_cell,
                                     float* query_heatmap_score, float* query_feat, float* query_pos, void* stream)
{
    AL3D_REQUIRE(B >= 0 && H > 0 && W > 0 && C >= 1 && C <= 32 && P >= 1 && P <= TP_MAXP && hidden >= 1,
                 "al3d_tf_proposals_f32: bad sizes (1 <= classes <= 32, 1 <= proposals <= 256)");
    AL3D_REQUIRE(nms_kernel >= 1 && (nms_kernel & 1) && nms_kernel / 2 < H && nms_kernel / 2 < W, "al3d_tf_proposals_f32: odd nms kernel");
    AL3D_REQUIRE((int64_t)H * W * C < (1ll << 31) && (int64_t)H * W * C >= P, "al3d_tf_proposals_f32: grid too large / fewer cells than proposals");
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(heat_logits && tokens && bev_pos && class_cols && class_bias && workspace && top_class && top_cell &&
                 query_heatmap_score && query_feat && query_pos, "al3d_tf_proposals_f32: null pointer");
    hipStream_t s = (hipStream_t)stream;
    unsigned* keys = (unsigned*)workspace;
    hipLaunchKernelGGL(tp_peak_kernel, dim3((unsigned)al3d_cdiv((int64_t)B * H * W, 256)), dim3(256), 0, s, heat_logits, B, H, W, C,
                       nms_kernel, free_class_mask, keys);
    hipLaunchKernelGGL(tp_select_kernel, dim3((unsigned)B), dim3(TP_THREADS), 0, s, keys, H * W, C, P, tokens, hidden, bev_pos,
                       class_cols, class_bias, top_class, top_cell, query_heatmap_score, query_feat, query_pos);
    AL3D_CHECK_LAUNCH("al3d_tf_proposals_f32");
    return AL3D_OK;
}
