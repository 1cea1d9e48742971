// doc_feed.hip -- the id-fed batch: the doc split's documents are a function of the user / item id
// (preprocess/divide_and_create_example_doc.py:261-262 stores meta.pkl's per-id documents in every example), so a batch is
// (u_id, i_id, rating) and its documents are gathered on the device from int32 tables resident there, instead of the
// 2 x B x L int64 tokens and two bool masks that the reference's collate builds on the host (trainer/train_deepconn_pp.py:281-292).
//
//   docs_out[r, :] = table[id_r, :]  (rows [0, B): user_docs by u_ids, rows [B, 2B): item_docs by i_ids; int32 -> int64)
//   masks_out      = docs_out != pad_token                                                 (utils.py:30-42, get_mask)
//   ids_out[r]     = id_r
// An id outside its table is never dereferenced: row `replace_id` stands in for it, ids_out gets `replace_id`, and err is
// updated as rbr::sanitize_id does (feed_ids.h: the convention review_feed.hip shares).
#include "rbr_common.h"
#include "feed_ids.h"

namespace rbr {

struct DocGather {
    FeedIds F;
    const int* table[2];
    long long* docs;
    unsigned char* masks;
    long long pad;
    int B, L;
};

// L % 4 == 0: one 4-token chunk per lane -- a 16-byte load of int32 tokens, two 16-byte int64 stores, one 4-byte mask store
__global__ __launch_bounds__(256) void doc_gather_vec_kernel(const DocGather G, long long* __restrict__ err) {
    const int cpr = G.L >> 2;                         // chunks per row
    const long long n = 2LL * G.B * cpr;
    for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < n; c += (long long)gridDim.x * 256) {
        const int r = (int)(c / cpr), q = (int)(c - (long long)r * cpr);
        int side;
        const long long id = feed_row_id(G.F, r, side, q == 0, err);
        const int4 t = *reinterpret_cast<const int4*>(G.table[side] + id * G.L + 4 * q);
        longlong2* d = reinterpret_cast<longlong2*>(G.docs + c * 4);
        d[0] = make_longlong2(t.x, t.y);
        d[1] = make_longlong2(t.z, t.w);
        if (G.masks) {
            const unsigned m = (unsigned)((long long)t.x != G.pad) | ((unsigned)((long long)t.y != G.pad) << 8) |
                               ((unsigned)((long long)t.z != G.pad) << 16) | ((unsigned)((long long)t.w != G.pad) << 24);
            reinterpret_cast<unsigned*>(G.masks)[c] = m;
        }
    }
}

// any L (odd, 1, unaligned pointers): one token per lane
__global__ __launch_bounds__(256) void doc_gather_scalar_kernel(const DocGather G, long long* __restrict__ err) {
    const long long n = 2LL * G.B * G.L;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int r = (int)(e / G.L), j = (int)(e - (long long)r * G.L);
        int side;
        const long long id = feed_row_id(G.F, r, side, j == 0, err);
        const long long t = G.table[side][id * G.L + j];
        G.docs[e] = t;
        if (G.masks) G.masks[e] = t != G.pad;
    }
}

}  // namespace rbr

extern "C" int rbr_doc_gather(int32_t B, int32_t L, const int64_t* u_ids, const int64_t* i_ids, const int32_t* user_docs, int32_t U,
                              const int32_t* item_docs, int32_t I, int64_t pad_token, int64_t replace_id, int64_t* docs_out,
                              uint8_t* masks_out, int64_t* ids_out, int64_t* err, void* stream) {
    using namespace rbr;
    if (B <= 0 || L <= 0 || U <= 0 || I <= 0) { set_error("rbr_doc_gather: bad shape B=%d L=%d U=%d I=%d", B, L, U, I); return RBR_ERR_BAD_ARG; }
    if (!u_ids || !i_ids || !user_docs || !item_docs || !docs_out || !err) { set_error("rbr_doc_gather: null pointer"); return RBR_ERR_BAD_ARG; }
    if (replace_id < 0 || replace_id >= U || replace_id >= I) {
        set_error("rbr_doc_gather: replace_id %lld is not a row of both tables (U=%d, I=%d)", (long long)replace_id, U, I);
        return RBR_ERR_BAD_ARG;
    }
    DocGather G;
    G.F.ids[0] = reinterpret_cast<const long long*>(u_ids); G.F.ids[1] = reinterpret_cast<const long long*>(i_ids);
    G.F.rows[0] = U; G.F.rows[1] = I;
    G.F.ids_out = reinterpret_cast<long long*>(ids_out);
    G.F.replace = replace_id;
    G.F.B = B;
    G.table[0] = user_docs; G.table[1] = item_docs;
    G.docs = reinterpret_cast<long long*>(docs_out);
    G.masks = masks_out;
    G.pad = pad_token;
    G.B = B; G.L = L;
    hipStream_t st = (hipStream_t)stream;
    const auto aligned = [](const void* p, uintptr_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % a) == 0; };
    const bool vec = L % 4 == 0 && aligned(user_docs, 16) && aligned(item_docs, 16) && aligned(docs_out, 16) && aligned(masks_out, 4);
    const long long work = vec ? 2LL * B * (L / 4) : 2LL * B * L;
    const unsigned grid = (unsigned)std::min<long long>((work + 255) / 256, 1LL << 20);     // grid-stride beyond 2^28 lanes
    if (vec)
        hipLaunchKernelGGL(doc_gather_vec_kernel, dim3(grid), dim3(256), 0, st, G, reinterpret_cast<long long*>(err));
    else
        hipLaunchKernelGGL(doc_gather_scalar_kernel, dim3(grid), dim3(256), 0, st, G, reinterpret_cast<long long*>(err));
    RBR_CHECK_LAUNCH("doc_gather launch");
    return 0;
}
