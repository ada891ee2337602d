/*
 * vlsat.h -- C ABI of libvlsat_hip.so: the MI355X (gfx950) implementation of VL-SAT's
 * per-scene eval forward.
 *
 * The reference has NO native/FFI layer (pure Python on PyTorch + PyG); its boundary for this
 * path is the nn.Module call
 *     Mmgnet.forward(obj_points, obj_2d_feats, edge_indices, descriptor, batch_ids, istrain=False)
 *         reference src/model/SGFN_MMG/model.py:288-335, called from process_val :458-460,
 *         which MMGNet.validation calls at src/model/model.py:203-211.
 * Every entry point below replaces a piece of that call; the reference line it stands for is
 * cited on each declaration.  The ctypes binding a reference maintainer would add is shown in
 * INTEGRATION.md and implemented in cvpr2023-vlsat_amd/lib.py.
 *
 * Conventions
 *   - plain pointers and sizes only; device pointers are raw HIP device addresses
 *     (torch: tensor.data_ptr()); `stream` is a hipStream_t passed as void*
 *     (torch: torch.cuda.current_stream().cuda_stream); NULL = the default stream.
 *   - all tensors fp32 row-major contiguous unless noted; indices int64 like the reference.
 *   - every function returns 0 on success or a negative VLSAT_E* code; it never throws and
 *     never calls exit(); vlsat_last_error() returns a thread-local message for the last failure.
 *   - vlsat_forward and the vlsat_k_* kernels are asynchronous on `stream` and do not synchronise.
 *   - vlsat_plan_create / vlsat_plan_destroy never wait for the device either: the index tables are uploaded
 *     asynchronously from pinned memory and the first forward of the plan waits for them ON THE DEVICE; a destroyed
 *     plan's workspace is recycled behind the event of its last forward.  Device-wide waits exist only in
 *     vlsat_load_weight (when it replaces an already finalised set), vlsat_set_gemm_precision, vlsat_destroy and the
 *     vlsat_debug_* readers.
 *   - a handle (weights) may be shared by several plans; a plan owns its workspace and is NOT
 *     re-entrant (one forward at a time per plan; ), mirroring one nn.Module instance; a handle is driven from one
 *     host thread at a time, and its forwards are ordered on ONE stream at a time (small scratch buffers -- the split-K
 *     workspace of small GEMM launches -- belong to the handle: moving to another stream needs an event / sync between
 *     the last forward on the old stream and the first on the new one; separate handles are independent).
 *   - several handles may be driven from several host threads at the same time (one thread and one stream per handle:
 *     evaluate.validation(workers=K)).  The forward path launches only kernels of this library -- no hipMemsetAsync, no
 *     runtime device-to-device copy: a hipMemsetAsync issued from several threads at once was caught writing a foreign
 *     pattern about once per 20 000 calls.  A host that drives handles from threads should keep
 *     runtime fills (and library reductions that use them internally) out of those threads as well.
 */
#ifndef VLSAT_H
#define VLSAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLSAT_OK            0
#define VLSAT_EINVAL       (-1)   /* bad argument / shape */
#define VLSAT_EHIP         (-2)   /* HIP runtime error (message has hipGetErrorString) */
#define VLSAT_ESTATE       (-3)   /* call order (weights missing / not finalised) */
#define VLSAT_EGRAPH       (-4)   /* graph layout not supported as given (see vlsat_plan_create) */
#define VLSAT_ENOMEM       (-5)

typedef struct vlsat_ctx*  vlsat_handle;
typedef struct vlsat_plan_s* vlsat_plan;

/* Hyper-parameters = the MODEL keys Mmgnet.__init__ reads (reference SGFN_MMG/model.py:26-130,
 * config/mmgnet.json:26-58). */
typedef struct {
    int32_t n_layers;        /* MODEL.N_LAYERS */
    int32_t n_heads;         /* MODEL.NUM_HEADS (8); built: 4, 8, 16 */
    int32_t dim_atten;       /* MODEL.DIM_ATTEN (256); built: 128, 256, 512 */
    int32_t gcn_aggr;        /* MODEL.GCN_AGGR: 0 max, 1 add, 2 mean */
    int32_t dim_point;       /* 3, +3 with MODEL.USE_RGB, +3 with MODEL.USE_NORMAL (SGFN_MMG/model.py:31-35) */
    int32_t n_obj_class;     /* 160 */
    int32_t n_rel_class;     /* 26 (27 in the single-label setting) */
    float   obj_logit_scale; /* log(1/0.07): never checkpointed by the reference */
    int32_t use_gcn_edge;    /* MODEL.USE_GCN_EDGE (1): gate MLP on cat[q,k]; 0: on q alone (network_MMG.py:72-75) */
    int32_t multi_rel_outputs; /* MODEL.multi_rel_outputs (1): sigmoid relation head; 0: log_softmax (SGFN_MMG/model.py:113-130) */
    int32_t feature_transform; /* MODEL.feature_transform (0): STNkd 64x64 transform after conv1 of the three encoders */
    /* MODEL.WITH_BN needs no field: the relation heads' bn1/bn2 tensors are folded when the checkpoint has them */
} VlsatDims;

const char* vlsat_last_error(void);
/* library / build identification, e.g. "vlsat-hip gfx950 r4 (fp32-mfma | bf16x3 | bf16_mixed | bf16)" */
const char* vlsat_version(void);

/* Mmgnet.__init__ (module construction), reference SGFN_MMG/model.py:20-159. */
int vlsat_create(const VlsatDims* dims, vlsat_handle* out);
void vlsat_destroy(vlsat_handle h);

/* BaseModel.load / load_state_dict, reference model_utils/model_base.py:75-129: `name` is the
 * reference state_dict key prefixed by the sub-module name ("mmg.gcn_3ds.0.edgeatten.nn_edge.0.weight");
 * `host` is fp32, `count` elements.  Unknown names -> VLSAT_EINVAL.  Like BaseModel.load, loading may be repeated:
 * the first call after a vlsat_finalize_weights starts a new, complete set (it waits for the device to go idle and
 * drops the previous device tensors); existing plans stay valid.  "triplet_projector_2d.{0,3}.{weight,bias}" are
 * optional and only read by vlsat_forward_train. */
int vlsat_load_weight(vlsat_handle h, const char* name, const float* host, size_t count);
/* Folds BatchNorm(eval), splits/concatenates/permutes the projections the kernels use and
 * uploads everything to the device.  Fails with VLSAT_ESTATE listing the first missing tensor. */
int vlsat_finalize_weights(vlsat_handle h);

/* Graph analysis for one batch = what MMG.forward derives from batch_ids each call
 * (reference network_MMG.py:183-205) plus the PyG gather/scatter index bookkeeping
 * (network_util.py:50-73).  HOST pointers: batch_ids [N] int64 (scene id per node, scenes
 * contiguous and ascending), edges [2,E] int64 (row 0 = source, row 1 = target, already offset
 * like collate_fn_mmg does, reference DataLoader.py:167-172).  Requirements: every edge joins two
 * nodes of one scene; edges of a scene are contiguous and scenes appear in node order
 * (otherwise VLSAT_EGRAPH: the Python glue then permutes edges and retries).  Within a scene the
 * edge order is arbitrary.  Allocates (or recycles) the per-plan device workspace for (N, E, P).  Returns without
 * waiting for the device; the host arrays may be freed as soon as it returns. */
int vlsat_plan_create(vlsat_handle h, const int64_t* batch_ids_host, const int64_t* edges_host,
                      int64_t n_nodes, int64_t n_edges, int32_t n_points, vlsat_plan* out);
void vlsat_plan_destroy(vlsat_plan p);
/* n_scenes, workspace bytes, and whether the fully-connected fast paths were selected */
int vlsat_plan_info(vlsat_plan p, int32_t* n_scenes, size_t* workspace_bytes, int32_t* is_fc);

/* Does a DEVICE copy of a graph equal what this plan was built from?  *mismatches (device int32, zeroed by the caller) receives
 * the number of columns of edges_dev ([2,E] int64, the layout Mmgnet.forward takes) that differ from the plan's edge list plus the
 * nodes at which batch_ids_dev ([N] int64, may be NULL) starts a new run where the plan has no scene boundary (or the reverse).
 * Asynchronous on `stream`; no host wait.  For hosts that name a graph by a key (e.g. the object counts of fully-connected
 * scenes) instead of handing the edge list over: one call per new key makes the key's claim checked -- a permuted edge list
 * would otherwise attribute every relation row to the wrong edge (reference edge order: src/dataset/dataset_3dssg.py:264-266). */
int vlsat_plan_check_graph(vlsat_plan p, const int64_t* edges_dev, const int64_t* batch_ids_dev, int32_t* mismatches, void* stream);

/* Mmgnet.forward(..., istrain=False), reference SGFN_MMG/model.py:288-335.
 * Device pointers: obj_points [N,dim_point,P], obj_2d_feats [N,512], descriptor [N,11];
 * outputs obj_logits_3d/2d [N,n_obj_class] (logits x exp(scale)), rel_cls_3d/2d
 * [E,n_rel_class] (post-sigmoid; log_softmax when multi_rel_outputs = 0).  Edge order of the outputs = edge
 * order given to the plan.
 * 3D-only mode: pass NULL for BOTH obj_logits_2d and rel_cls_2d (obj_2d_feats may then be NULL too):
 * the whole 2D branch is skipped -- exact, because the 3D branch never reads 2D tensors. */
int vlsat_forward(vlsat_handle h, vlsat_plan p,
                  const float* obj_points, const float* obj_2d_feats, const float* descriptor,
                  float* obj_logits_3d, float* obj_logits_2d, float* rel_cls_3d, float* rel_cls_2d,
                  void* stream);

/* Mmgnet.forward(..., istrain=True) in eval mode (no dropout, no autograd), reference SGFN_MMG/model.py:291-292,312,
 * 319-322,332-333: the four outputs of vlsat_forward plus obj_feature_3d_mimic [N,512] (first 512 columns of the
 * point encoder's output), obj_features_2d_mimic [N,512] (the adapter's output) and gcn_edge_feature_2d_dis [E,512]
 * (triplet_projector_2d on cat[x2[ei[0]], x2[ei[1]], e2]); the tuple's eighth element is exp(dims.obj_logit_scale).
 * Needs the triplet_projector_2d weights. */
int vlsat_forward_train(vlsat_handle h, vlsat_plan p,
                        const float* obj_points, const float* obj_2d_feats, const float* descriptor,
                        float* obj_logits_3d, float* obj_logits_2d, float* rel_cls_3d, float* rel_cls_2d,
                        float* obj_feature_3d_mimic, float* obj_features_2d_mimic, float* gcn_edge_feature_2d_dis,
                        void* stream);


/* Operand precision of the matrix kernels inside vlsat_forward (BASELINE configs[2], "bf16 MFMA for the
 * QKV/FFN GEMMs"): 0 = fp32 (default; BASELINE configs[1]): fp32 MFMA on the node-row, tail and small GEMM launches, the gate and the
 * encoders; the full rounds of the large edge-row GEMM launches (256 x 256 8-phase kernel) as three fp16 MFMAs per product into an fp32
 * accumulator -- fp32 tensors in and out, A split in registers into fp16 hi + (lo 2^11), the weights as fp16 planes of W 2^k (k per
 * tensor, made when the weights are finalised; vlsat_gemm.h), 0.3 to 1.3 times the exact kernel's error against fp64; domain
 * |A| <= 65504 (beyond, the operand saturates and results stay finite), weights below 2^-16 of their tensor's largest lose low bits;
 * vlsat_debug_option "gemm_exact" 1 restores the exact fp32-MFMA kernels; the edge
 * cross-attention's products (head dim 64) as three fp16 MFMAs each (operands split into fp16 hi + lo, 2^-22), fp32 accumulate and
 * softmax -- 1.1 to 2 times the exact kernel's error, far inside 1e-4 on the outputs; domain |Q / sqrt(d_k) * log2 e|, |K| < 65504 and, V
 * being multiplied by 2^3 before the split, |V| < 65504 / 8 = 8188 (values beyond are clamped there);
 * vlsat_debug_option "flash_exact" 1 restores the exact fp32-MFMA attention kernel; 3 = split-bf16 (a_hi.w_hi + a_lo.w_hi +
 * a_hi.w_lo on v_mfma_f32_32x32x16_bf16, fp32 accumulate, ~1e-5 error); 1 = single-rounded bf16 operands
 * everywhere (~2e-2 on the x14.29 object logits: outside the config's 1e-2); 2 = mixed: single-rounded bf16 on the
 * edge-row GEMMs / attention / gate and split-bf16 on the node-row GEMMs (meets 1e-2 at Xavier-scale weights);
 * 4 = split-bf16 everywhere except the edge cross-attention (reference network_MMG.py:228-234: its q / k|v / out projections and the
 * attention itself), which is single-rounded -- the 3D outputs never read that block and keep mode 3's accuracy, the 2D outputs hold
 * 1e-2 on weights where mode 2 does not;
 * 5 = mode 2 on FP16: the half-row tensors between the edge-row kernels hold fp16 instead of bf16 and those kernels (8-phase / ring / small
 * GEMMs, edge attention, gate, PointNet) run v_mfma_f32_32x32x16_f16 -- the bf16 rate on CDNA4, 2^-12 instead of 2^-9 per stored value and
 * operand: 7e-4 where mode 2 has 5e-3, 3-4 % slower (the chip is power-limited and fp16 multipliers draw more); values beyond +-65504 saturate.
 * Activations in HBM, softmax and LayerNorm stay fp32 in every mode.  May be changed between forwards; the bf16
 * planes of the weights are made inside this call (it waits for the device), never inside a forward. */
int vlsat_set_gemm_precision(vlsat_handle h, int32_t mode);

/* Which 3D edges a 2D edge attends to in the edge cross-attention (reference network_MMG.py:228-234), for plans
 * created AFTER the call.  0 (default): the edges of its own scene -- validation()'s contract, which runs one scene
 * per call (src/model/model.py:185).  1: every edge of the batch -- what the reference computes when a single call
 * carries several scenes, because that attention has no scene mask; the 3D outputs are identical in
 * both modes, the 2D outputs are not. */
int vlsat_set_edge_attention_scope(vlsat_handle h, int32_t scope);

/* Per-kernel timing of the forward with HIP events on `stream` (bench.py roofline leg).
 * enable=1: every launch of every kernel class is bracketed by hipEventRecord on the launch
 * stream; vlsat_profile_read synchronises, accumulates and returns per-class totals since
 * the last read.  Classes are enumerated by vlsat_profile_class_name(i), i in [0, n). */
int vlsat_profile_enable(vlsat_handle h, int32_t enable);
int vlsat_profile_num_classes(void);
const char* vlsat_profile_class_name(int32_t cls);
int vlsat_profile_read(vlsat_handle h, int32_t cls, double* total_ms, int64_t* launches, double* flops);

/* -------- single-kernel entry points (unit/parity tests; all device pointers) ---------------- */

/* C[M,N] = act(rowscale[m] * (reluA?(A)[M,K] . W[N,K]^T) + bias[n] + resid_scale*resid[m,n]
 *              + g0[gi0[m], n] + g1[gi1[m], n]);   act: 0 none, 1 relu, 2 sigmoid.
 * Replaces every nn.Linear / Conv1d(k=1) call site of the path (SURVEY §2 "addmm" row).
 * K % 32 == 0; lda/ldw % 4 == 0; any pointer except A, W, C may be NULL; rowscale may not be
 * combined with resid/g0/g1 (VLSAT_EINVAL). */
int vlsat_k_gemm(const float* A, int32_t lda, const float* W, int32_t ldw, float* C, int32_t ldc,
                 int32_t M, int32_t N, int32_t K,
                 const float* bias, const float* rowscale,
                 const float* resid, int32_t ldr, float resid_scale,
                 const float* g0, const int32_t* gi0, int32_t ldg0,
                 const float* g1, const int32_t* gi1, int32_t ldg1,
                 int32_t relu_a, int32_t act, void* stream);

/* Weight planes of the bf16 modes: w[i] ~= bf16 hi[i] + bf16 lo[i] (asynchronous on `stream`). */
int vlsat_k_split_bf16(const float* w, size_t n, uint16_t* hi, uint16_t* lo, void* stream);

/* vlsat_k_gemm on the bf16 matrix cores (BASELINE configs[2]) with caller-provided planes of W (dense [N,K], ldw = K):
 * prec 1 = single-rounded bf16 operands, 3 = split-bf16 (three MFMAs per product).  A stays fp32 and is split inside
 * the kernel.  no_dma = 1: the VGPR-staged operand pipe of round 1 instead of the LDS-direct one; prefetch: slices of
 * look-ahead of the A-panel prefetch (0 = off, -1 = default).  fmt: bit 0 = A, bit 1 = resid, bit 2 = C are in the
 * split-pair format of the split-bf16 mode (one 32-bit word per element: bf16 hi = rne(x) in the upper half, bf16 lo =
 * rne(x - hi) in the lower half) or, with bit 5 set, in the half-row format of the single-rounding modes (bf16 values
 * at byte 2 * column of the fp32-pitched row; prec 1 only); bit 3: g0 / g1 are FP16 half rows (fp16 values at byte 2 * column of the
 * fp32-pitched table row; no residual, N % 256 == 0), bits 25..28: k = that many times 256 leading columns of C are written as fp16 half
 * rows, clamped to +-65504 (the node-side projection's [P_i | P_j], which nn_edge.0 gathers per edge); bits 4 / 6 / 7 are benchmarking switches (
 * no ring kernel, small launches on the split-K kernel, ring kernel with 128 x 256 tiles; bits 10 / 11: its
 * 32-wide k slices / single fragment set in the half-row mode) and bits 8 / 9 timing
 * ablations (no operand loads / no MFMAs: garbage results); c_scale multiplies C
 * last.  Asynchronous. */
int vlsat_k_gemm_planes(const float* A, int32_t lda, const float* W, const uint16_t* Whi, const uint16_t* Wlo, int32_t ldw,
                        float* C, int32_t ldc, int32_t M, int32_t N, int32_t K, const float* bias,
                        const float* resid, int32_t ldr, float resid_scale,
                        const float* g0, const int32_t* gi0, int32_t ldg0,
                        const float* g1, const int32_t* gi1, int32_t ldg1,
                        int32_t relu_a, int32_t act, int32_t prec, int32_t no_dma, int32_t prefetch, int32_t fmt,
                        float c_scale, void* stream);
/* Test entry point: the same with the planes made on the spot from W (allocates, synchronises). */
int vlsat_k_gemm_bf16(const float* A, int32_t lda, const float* W, int32_t ldw, float* C, int32_t ldc,
                      int32_t M, int32_t N, int32_t K, const float* bias,
                      const float* resid, int32_t ldr, float resid_scale,
                      const float* g0, const int32_t* gi0, int32_t ldg0,
                      const float* g1, const int32_t* gi1, int32_t ldg1,
                      int32_t relu_a, int32_t act, int32_t prec, int32_t no_dma, void* stream);

/* PointNetfeat.forward (obj_encoder), reference network_PointNet.py:141-164:
 * pts [N,3,P] -> out [N,768] = max_p relu(W3 relu(W2 relu(W1 x + b1) + b2) + b3).
 * Weights in the reference layout (W1 [64,3], W2 [128,64], W3 [768,128]). */
int vlsat_k_pointnet(const float* pts, int32_t n_obj, int32_t n_points,
                     const float* w1, const float* b1, const float* w2, const float* b2,
                     const float* w3, const float* b3, int32_t n_out, float* out, void* stream);

/* ScaledDotProductAttention core for the edge cross-attention (reference attention.py:60-76 as
 * called from network_MMG.py:231): per scene s and head h, O = softmax(Q K^T * scale) V with
 * Q,K,V,O [T,512] (head h = columns 64h..64h+63), tokens of scene s = rows tok_ptr[s]..tok_ptr[s+1].
 * tok_ptr is a HOST array of n_scenes+1 int64.  Never materialises the T x T scores. */
int vlsat_k_flash_attn(const float* Q, const float* K, const float* V, float* O,
                       int32_t ld, const int64_t* tok_ptr_host, int32_t n_scenes, int32_t n_heads,
                       float scale, void* stream);

/* The same attention on the bf16 matrix cores (BASELINE configs[2]): terms = 3 split-bf16 (three MFMAs per product,
 * ~1e-5) or 1 (single-rounded operands); use_tr = 1 reads the V operand with the LDS transpose read, 0 gathers it,
 * 2 = transpose read with Q (pre-multiplied by scale*log2 e), K, V and O in the split-pair format, 3 = the same in the
 * half-row format (terms = 1). */
int vlsat_k_flash_attn_bf16(const float* Q, const float* K, const float* V, float* O,
                            int32_t ld, const int64_t* tok_ptr_host, int32_t n_scenes, int32_t n_heads,
                            float scale, int32_t terms, int32_t use_tr, void* stream);

/* LayerNorm over rows of 512 in place, optional ReLU (reference attention.py:122 + MMG :236-248). */
int vlsat_k_layernorm(float* x, int32_t ld, int32_t rows, int32_t dim, const float* gamma,
                      const float* beta, int32_t relu, void* stream);

/* The 'fat' gate of MultiHeadedEdgeAttention.forward (reference network_MMG.py:96-104): per (edge e, head h)
 *     hidden = relu(Gq[src[e], h, :] + W0k . kproj[e, h, :]);  prob = softmax(W3 . hidden + b3);  gated = prob * value[dst[e], h, :]
 * on the operands the forward prepares: kproj [E, H*dk] = proj_edge output HEAD-MAJOR (column h*dk + c
 * is the reference's k.view(E,dk,H)[e,c,h]); `node` = the node-side buffer with row pitch ld_node holding, at column gq_off,
 * Gq[n, h*2dk + o] = b0[o] + sum_c W0[o,c] q.view(N,dk,H)[n,c,h] (the query half of nn.0 applied per node, bias included)
 * and, at column v_off, value[n, h*dox + m] = proj_value output head-major; src / dst [E] int32 (ei[0] / ei[1]);
 * w0k [2dk, dk] = nn.0.weight[:, dk:2dk], w3 [dox, 2dk] = nn.3.weight, b3 [dox].  Outputs: gated [E, H*dox] head-major
 * (column h*dox + m; the reference's is m*H + h) and, if not NULL, prob [E, dox, H] in the REFERENCE layout.
 * use_edge = 0: MODEL.USE_GCN_EDGE false (hidden = relu(Gq), kproj / w0k unread).  ld_node, gq_off, v_off % 4 == 0.
 * variant: 0 = the exact fp32 kernel of the geometry, 1 = VALU kernel (any geometry), 2 = fp32 MFMA template
 * (NUM_HEADS in {4,8,16} x DIM_ATTEN in {128,256,512}), 3 / 4 = bf16 matrix cores, split-bf16 / single-rounded (kproj fp32),
 * 5 = the split-fp16 kernel the fp32 forward runs at 8 heads x (64, 32): three fp16 MFMAs per product, fp32 tensors in and out,
 * raw fp32 weights (the kernel makes its planes itself); any other geometry is VLSAT_EINVAL.
 * All device pointers; asynchronous. */
int vlsat_k_edge_gate(const float* kproj, const float* node, int32_t ld_node, int32_t gq_off, int32_t v_off,
                      const int32_t* src, const int32_t* dst, const float* w0k, const float* w3, const float* b3,
                      float* gated, float* prob, int32_t n_edges, int32_t n_heads, int32_t dk, int32_t dox,
                      int32_t use_edge, int32_t variant, void* stream);

/* Aggre_Index (reference network_util.py:64-73, torch_scatter semantics): out[n, col0 + c] = reduce over the rows e of
 * gated [E, n_ch] (dense) with index[e] == n; aggr 0 max | 1 add | 2 mean (MODEL.GCN_AGGR); empty segment -> 0.
 * index_host: HOST int64 [E] (ei[0] under flow = target_to_source).  Deterministic (CSR, no atomics).  Synchronises. */
int vlsat_k_aggregate(const float* gated, int32_t n_ch, const int64_t* index_host, int64_t n_edges, int32_t n_nodes,
                      int32_t aggr, float* out, int32_t ldo, int32_t col0, void* stream);

/* ScaledDotProductAttention core of the node self / cross attention (reference attention.py:60-76 as called from
 * network_MMG.py:217-218) with the additive distance bias and the block-diagonal scene mask of network_MMG.py:188-203:
 * per scene s, head h: O = softmax(scale * Q K^T + bias[s,h]) V over the scene's nodes; head h = columns h*dk.. of Q/K/V/O
 * with dk = 512 / n_heads in {32, 64, 128}.  node_ptr_host: HOST int64 [n_scenes+1]; bias (may be NULL): scene s at float
 * offset sum_{t<s} H n_t^2, layout [H][n_s][n_s] (query-major) -- what vlsat_k_dist_bias writes.  lanes_per_query: 0 = the
 * forward's choice, 1 / 16 = force the one-query-per-lane / sixteen-lanes-per-query kernel.  Synchronises. */
int vlsat_k_node_attn(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv,
                      float* O, int32_t ldo, const float* bias, const int64_t* node_ptr_host, int32_t n_scenes,
                      int32_t n_heads, float scale, int32_t lanes_per_query, void* stream);

/* The distance-bias MLP MMG.forward runs once per call (reference network_MMG.py:190-203, self_attn_fc :165-173):
 * bias[s][h][a][b] = Linear(32,H)(LN(relu(Linear(32,32)(LN(relu(Linear(4,32)([c_b - c_a, |c_b - c_a|]))))))) for the nodes a, b
 * of scene s; c = desc[:, 0:3] (row pitch ld_desc).  Weights in the reference layout (self_attn_fc.{0,2,3,5,6}).
 * Output layout as vlsat_k_node_attn reads it.  Synchronises. */
int vlsat_k_dist_bias(const float* desc, int32_t ld_desc, const int64_t* node_ptr_host, int32_t n_scenes, int32_t n_heads,
                      const float* w0, const float* b0, const float* ln2_w, const float* ln2_b, const float* w3,
                      const float* b3, const float* ln5_w, const float* ln5_b, const float* w6, const float* b6,
                      float* bias, void* stream);

/* vlsat_k_pointnet for every encoder kernel and operand form: pts [N,cin,P] with cin in {3, 6, 9} (W1 [64,cin]), n_out a
 * multiple of 128 up to 768.  terms: 0 = the fp32 kernel; 1 / 2 / 3 = the matrix-core kernel of the 16-bit modes with conv2 /
 * conv3 operands as single-rounded bf16 / single-rounded fp16 (clamped to +-65504) / split bf16 (hi + lo, three MFMAs per
 * product); 5 = the same kernel as the fp32 precision mode runs it: split fp16 -- activations as fp16 hi + (lo 2^11), clamped to 65504,
 * the weights as the planes of vlsat_k_split_f16s, three f16 MFMAs per product, the exact kernel's error against fp64 (4 is refused);
 * conv1, the biases, the ReLUs and the max stay fp32.  The planes of W2 / W3 are made on the spot from the fp32
 * weights (terms != 0: allocates, synchronises). */
int vlsat_k_pointnet_ex(const float* pts, int32_t n_obj, int32_t n_points, int32_t cin,
                        const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* w3, const float* b3, int32_t n_out, int32_t terms, float* out, void* stream);

/* vlsat_k_layernorm in every form the forward uses: y[r, :] = LN(x[r, :] + resid[r, :]) over rows of 512 (row pitches ld,
 * ldy, ldr in floats, multiples of 4; y may be x or resid).  x_f16 = 1: the rows of x are fp16 half rows (fp16 values at
 * byte 2 * column).  resid may be NULL; resid_fmt: 0 fp32, 1 split-pair words, 2 bf16 half rows, 4 fp16 half rows.
 * out_fmt: 0 fp32, 1 split-pair words, 2 bf16 half rows, 4 fp16 half rows clamped to +-65504 (a half row fills the first
 * 1024 bytes of the row of y), 6 GEMM pair words of the fp32 mode (Ah << 16 | Al, Ah = f16(yc), Al = f16((yc - Ah) 2^11), yc = y
 * clamped to +-65504: csrc/gemm_f16s_planes.h; one word per element).  Any other out_fmt or x_f16 is refused.  Asynchronous. */
int vlsat_k_layernorm_to(const float* x, int32_t ld, float* y, int32_t ldy, int32_t rows, int32_t dim,
                         const float* gamma, const float* beta, int32_t relu, int32_t out_fmt,
                         const float* resid, int32_t ldr, int32_t resid_fmt, int32_t x_f16, void* stream);

/* Gen_edge_descriptor (reference src/utils/op_utils.py:78-97, flow target_to_source) + conv1 of both relation encoders:
 * ed = [desc[src, 0:6] - desc[dst, 0:6], log(desc[src, 6:11] / desc[dst, 6:11])], h1[e, c] = relu(w1cat[c, :] . ed + b1cat[c])
 * with desc [N,11], src / dst int32 [E], w1cat [128,11] (rows 0..63 rel_encoder_3d.conv1, 64..127 rel_encoder_2d.conv1),
 * h1 [E,128].  Asynchronous. */
int vlsat_k_edge_embed(const float* desc, const int32_t* src, const int32_t* dst, int32_t n_edges,
                       const float* w1cat, const float* b1cat, float* h1, void* stream);

/* Spatial tail of the 3D node feature (reference SGFN_MMG/model.py:296-299):
 * x[n, col0:col0+8] = [desc[n, 3:9], log desc[n, 9], log desc[n, 10]], row pitch ldx.  Asynchronous. */
int vlsat_k_desc_tail(const float* desc, int32_t n_nodes, float* x, int32_t ldx, int32_t col0, void* stream);

/* out[m] = scale / ||x[m, 0:512]||_2 (object heads, reference SGFN_MMG/model.py:327-330); x2 / out2 (both or neither): a
 * second problem of the same shape in the same launch.  Asynchronous. */
int vlsat_k_row_invnorm(const float* x, int32_t ld, int32_t rows, int32_t dim, float scale, float* out,
                        const float* x2, float* out2, void* stream);

/* dst[r, 0:cols] = src[r, 0:cols] for r < rows (pitches in floats): the forward's device-to-device copy; 16-byte accesses
 * when cols, both pitches and both pointers allow, scalar ones otherwise.  Asynchronous. */
int vlsat_k_copy_rows(float* dst, int64_t dst_ld, const float* src, int64_t src_ld, int32_t cols, int64_t rows,
                      void* stream);

/* The glue of MODEL.feature_transform (STNkd, reference network_PointNet.py:52-86,146-150):
 * pts_conv1_rows: rows[n*P + p, c] = relu(b1[c] + sum_k w1[c,k] pts[n,k,p]), c < 64, cin in 1..9;
 * rowmax: out[n, c] = max_{p < P} x[n*P + p, c] for c < cols (row pitches ld / ldo);
 * apply_stn: out[r, j] = sum_i h[r, i] T[r / P][i, j] with T [n_obj,64,64].  Asynchronous. */
int vlsat_k_pts_conv1_rows(const float* pts, int32_t n_obj, int32_t n_points, int32_t cin,
                           const float* w1, const float* b1, float* rows, void* stream);
int vlsat_k_rowmax(const float* x, int32_t ld, int32_t n_obj, int32_t n_points, int32_t cols, float* out, int32_t ldo,
                   void* stream);
int vlsat_k_apply_stn(const float* h, int32_t ldh, const float* T, int64_t rows, int32_t n_points, float* out,
                      int32_t ldo, void* stream);

/* -------- input preparation (the step BEFORE the path: the data loader, reference dataset_3dssg.py:279-294) --- */

/* Per object n: gather P sampled points scene_points[choice[n, :]] ([Npts,3] fp32, choice int32 [N,P]),
 * descriptor[n] = gen_descriptor of them (reference src/utils/op_utils.py:47-64: centroid, unbiased std,
 * max-min, volume, max dim), obj_points[n] = the points minus their mean, laid out [N,3,P]
 * (zero_mean dataset_3dssg.py:189-191 + the permute of src/model/model.py:79).  All device pointers. */
int vlsat_prepare_objects(const float* scene_points, const int32_t* choice, int32_t n_obj, int32_t n_points,
                          float* obj_points, float* descriptor, void* stream);

/* Per-object point selection on the device -- the step in front of vlsat_prepare_objects (reference
 * src/dataset/dataset_3dssg.py:279-289: obj_pointset = points[np.where(instances == id)[0]]; choice = np.random.choice(len, P,
 * replace=True)).  instances int32 [Npts] (instance id of every scene point), instance_ids int32 [N] (the scene's objects, distinct,
 * each < map_size).  Builds every instance's point indices in ascending order (np.where's) by a stable segmented compaction and
 * draws n_sample of them with replacement from a counter-based generator: draw (obj, j) is a function of (seed, obj * n_sample + j)
 * only -- splitmix64 of seed + 0x9E3779B97F4A7C15 (obj n_sample + j + 1), top 32 bits scaled to the instance's point count
 * (csrc/prep.hip; oracle/prep_oracle.py restates it bit for bit; it is NOT numpy's Mersenne stream).  choice int32 [N, n_sample]
 * feeds vlsat_prepare_objects; counts int32 [N] = points per instance (0: the instance does not occur; its choices are 0).
 * id_map: int32 [map_size] scratch; scratch: int32 [vlsat_sample_objects_scratch(n_points, n_obj)].  Device pointers; asynchronous. */
size_t vlsat_sample_objects_scratch(int64_t n_points, int32_t n_obj);
int vlsat_sample_objects(const int32_t* instances, int64_t n_points, const int32_t* instance_ids, int32_t n_obj, int32_t n_sample,
                         uint64_t seed, int32_t* id_map, int32_t map_size, int32_t* scratch, int32_t* choice, int32_t* counts,
                         void* stream);

/* Fully-connected directed edges without self loops, source-major, for a batch of scenes with node
 * offsets applied, and the batch ids (dataset_3dssg.py:264-266 + collate_fn_mmg DataLoader.py:160-172).
 * node_ptr int32 [S+1] and edge_ptr int64 [S+1] (edge_ptr[s+1]-edge_ptr[s] = n_s(n_s-1)) are device arrays;
 * edges is [2,E] int64 (the layout Mmgnet.forward takes), batch_ids [N] int64. */
int vlsat_fc_edges(const int32_t* node_ptr, const int64_t* edge_ptr, int32_t n_scenes, int64_t n_nodes, int64_t n_edges,
                   int64_t* edges, int64_t* batch_ids, void* stream);

/* -------- proximity-pruned edge lists: the sparse alternative to vlsat_fc_edges for large scenes (csrc/proximity.hip) --------
 *
 * The rule (exact; prep.proximity_edges_host restates it in numpy, bit for bit):
 *   boxes f32 [N,6] = lo.xyz, hi.xyz: the unpadded axis-aligned box of ALL points of an instance (the reference pads the same box by
 *     0.2 per side, src/dataset/dataset_3dssg.py:286-288).  An instance without points has lo = +inf, hi = -inf.
 *   cand(i,j):  i != j, same scene, and on each of the three axes  lo_i[a] - padding < hi_j[a] + padding  and
 *     lo_j[a] - padding < hi_i[a] + padding  (strict; each side one fp32 operation).  An empty box is never a candidate.
 *   d(i,j):  g_a = max(0, max(lo_i[a] - hi_j[a], lo_j[a] - hi_i[a]));  d = (g_x*g_x + g_y*g_y) + g_z*g_z in fp32, every operation
 *     rounded to nearest on its own (no fused multiply-add), so d(i,j) and d(j,i) are the same bits.
 *   key_i(j) = (bits(d) << 32) | local index of j in its scene  (d >= 0, so the bit order is the value order; ties go to the lower index).
 *   keep_i(j):  key_i(j) is among the max_neighbors smallest keys over i's candidates.
 *   edge (i,j) is emitted iff cand(i,j) and (max_neighbors <= 0  or  keep_i(j)  or  keep_j(i)).
 * The list is symmetric ((i,j) present iff (j,i) is); a node's out-degree can EXCEED max_neighbors (it is kept by every node that
 * ranks it among its own nearest), and per scene E <= min(n(n-1), 2 n max_neighbors).  Order: scenes in node order, source-major,
 * targets ascending, node offsets applied -- the order of vlsat_fc_edges with the dropped pairs removed (a padding larger than the
 * scene and no cap give vlsat_fc_edges' output element for element).
 *
 * vlsat_instance_boxes: instances int32 [Npts], scene_points f32 [Npts,3], instance_ids int32 [N] (distinct, each < map_size; id_map is
 *   an int32 [map_size] scratch as in vlsat_sample_objects) -> boxes.  Points of other ids (background included) are ignored.  Exact:
 *   min / max by integer atomics on an order-preserving code of the float.
 * vlsat_proximity_count: node_ptr int32 [S+1] (device) -> edge_ptr int64 [S+1] and batch_ids int64 [N] in device memory, and the
 *   scratch (vlsat_proximity_scratch_bytes(N) bytes) that vlsat_proximity_fill reads.  The caller reads edge_ptr[S] (the one host
 *   wait), allocates edges int64 [2, capacity] and passes the count back as n_edges.
 * vlsat_proximity_fill: same boxes / node_ptr / padding / max_neighbors / scratch -> edges (row 0 = from, row 1 = to, row stride =
 *   capacity).  n_edges > capacity is VLSAT_EINVAL and nothing is written; no element at or beyond capacity of either row is written
 *   whatever n_edges says.  No global atomics; memory O(N + E), work O(sum n_s^2).
 * vlsat_proximity_lds_boxes: a block keeps the boxes of its rows' scenes in LDS up to this many, and reads global memory above it
 *   (same result).  All pointers are device pointers; the calls are asynchronous. */
int vlsat_instance_boxes(const int32_t* instances, const float* scene_points, int64_t n_points, const int32_t* instance_ids, int32_t n_obj,
                         int32_t* id_map, int32_t map_size, float* boxes, void* stream);
int32_t vlsat_proximity_lds_boxes(void);
size_t vlsat_proximity_scratch_bytes(int64_t n_nodes);
int vlsat_proximity_count(const float* boxes, const int32_t* node_ptr, int32_t n_scenes, int64_t n_nodes, float padding, int32_t max_neighbors,
                          void* scratch, int64_t* edge_ptr, int64_t* batch_ids, void* stream);
int vlsat_proximity_fill(const float* boxes, const int32_t* node_ptr, int32_t n_scenes, int64_t n_nodes, float padding, int32_t max_neighbors,
                         const void* scratch, int64_t n_edges, int64_t capacity, int64_t* edges, void* stream);

/* -------- annotation transfer onto a predicted segmentation (csrc/label_transfer.hip) --------
 *
 * Which annotated instance is a segment of the user's own segmentation?  The rule of the reference's data_processing/gen_data.py
 * (:196-216, :242-283 correspondence and counts, :312-349 decision), restated; prep.nearest_points_host / segment_overlap_host restate
 * it in numpy with the same operations, so every index, distance bit and count is equal.  The reference program itself cannot be run
 * (it needs open3d, trimesh and two modules that are not in its tree), so agreement with it is by reading, not by a recorded output.
 *
 * Nearest point (:249, :265-271).  For a predicted point q and an annotated point r:  d2 = (dx*dx + dy*dy) + dz*dz,  dx = q.x - r.x ...,
 *   in fp32, every operation rounded to nearest on its own (no fused multiply-add).  key(r) = (bits(d2) << 32) | index of r (d2 >= 0:
 *   the bit order is the value order; ties go to the lower index).  nn_index[q] = the index of the smallest key among the r with
 *   d2 <= max_sq_dist, nn_sqdist[q] = its d2; without one, nn_index = -1 and nn_sqdist = +inf.  max_sq_dist is a SQUARED distance: the
 *   reference compares Open3D's squared distance with its --max_dist (default 0.1).  A query with a non-finite coordinate has no
 *   correspondence; an annotated point with one is never returned.
 * Counts (:254-281).  size[s] = the number of ALL points of predicted segment s, with or without a correspondence.  count[s,g] = the
 *   number of its points whose nearest annotated point belongs to instance g, for the instances the caller lists in gt_ids: those that
 *   have a label other than 'none'.  Points that land on other instances count in size only.
 * Decision (:215, :315-346), in fp64 with the reference's operations.  A segment is considered iff size[s] > min_seg_size (strict;
 *   default 512).  ratio = count / size.  best = the instance with the largest count, ties to the lower instance id (a tie is never
 *   accepted: acceptance needs ratio > 0.5).  occ = ratio_second / ratio_best when at least occ_min_candidates instances have a
 *   non-zero count, else 0.  The default occ_min_candidates = 3 reproduces the reference's `len(list) > 2`, which lets a segment shared
 *   51 : 49 between exactly two instances pass; 2 is probably what was meant.  Accept iff ratio_best > corr_thres and occ < occ_thres
 *   (defaults 0.5 and 0.75, both strict).
 *
 * vlsat_nearest_points: query f32 [Q,3], ref f32 [G,3] -> nn_index int32 [Q], nn_sqdist f32 [Q].  Exact and deterministic: a uniform
 *   grid over the finite annotated points, built as a counting sort (bounding box by integer atomics on an order-preserving code of
 *   the float, per-cell histogram by int32 atomics, exclusive scan, fill), cell edge >= sqrt(max_sq_dist), at most 1024 cells per axis
 *   and 2^21 in all (the edge grows until the extent fits, which keeps the search of the 27 cells around a query exact).  The order of
 *   the points inside a cell varies from run to run, the result does not: every query takes the minimum of the 64-bit key.  Q = 0,
 *   G = 0 and max_sq_dist = 0 (exact coincidence only) are valid; a negative or NaN max_sq_dist is VLSAT_EINVAL.  scratch:
 *   vlsat_nearest_points_scratch_bytes(Q, G) bytes, 16-byte aligned.
 * vlsat_segment_overlap: pd_segments int32 [Q], nn_index int32 [Q], gt_instances int32 [G], segment_ids int32 [S] (distinct, each in
 *   [0, seg_map_size)), gt_ids int32 [n_gt] (distinct, each in [0, gt_map_size)); id_maps is an int32 [seg_map_size + gt_map_size]
 *   scratch (vlsat_segment_overlap_scratch_bytes; id -> slot tables as in vlsat_sample_objects) -> size [S], counts [S, n_gt],
 *   match [S] (the slot in gt_ids of the accepted instance, or -1), best / second [S] (the largest count and the largest among the
 *   other instances), n_candidates [S] (instances with a non-zero count).  Integer atomics only; the library reads nothing back.
 * All pointers are device pointers; the calls are asynchronous. */
size_t vlsat_nearest_points_scratch_bytes(int64_t n_query, int64_t n_ref);
int vlsat_nearest_points(const float* query, int64_t n_query, const float* ref, int64_t n_ref, float max_sq_dist, void* scratch,
                         int32_t* nn_index, float* nn_sqdist, void* stream);
size_t vlsat_segment_overlap_scratch_bytes(int32_t seg_map_size, int32_t gt_map_size);
int vlsat_segment_overlap(const int32_t* pd_segments, const int32_t* nn_index, int64_t n_query, const int32_t* gt_instances, int64_t n_ref,
                          const int32_t* segment_ids, int32_t n_seg, const int32_t* gt_ids, int32_t n_gt, int32_t* id_maps,
                          int32_t seg_map_size, int32_t gt_map_size, int32_t min_seg_size, double corr_thres, double occ_thres,
                          int32_t occ_min_candidates, int32_t* size, int32_t* counts, int32_t* match, int32_t* best, int32_t* second,
                          int32_t* n_candidates, void* stream);

/* -------- segments of an over-segmentation merged into objects along "same part" edges (csrc/segment_merge.hip) --------
 *
 * An over-segmentation splits every object into several segments; the data the reference generates for that setting joins the segments
 * of one object by the relation "same part" (NAME_SAME_PART, utils/define.py:26; built at data_processing/gen_data.py:467-481;
 * scan.inherit_relationships(..., same_part=...) emits it in both directions).  A model trained on such data predicts those edges; this
 * call consumes them: one node per object.  metrics.merge_segments_host restates the rule in numpy with the same operations, so every
 * table and every bit of the pooled probabilities is equal.
 *
 * Inputs (per batch, as for vlsat_graph_decode): obj_probs f32 [N,C]; rel_probs f32 [E,R], finite and non-negative (no -0); edges int64
 *   [E,2] node rows in ANY order, duplicates and self loops allowed; batch_ids int64 [N] or NULL (one scene), the nodes of a scene
 *   contiguous and scenes ascending; same_part in [0,R); threshold f32; mutual 0/1; weights f32 [N], positive, or NULL (all 1) -- the
 *   caller passes the points per segment.
 * Link.  Edge e = (a,b) is a link iff a != b, batch_ids[a] == batch_ids[b] and rel_probs[e,same_part] >= threshold (fp32 compare;
 *   equality passes).  With mutual = 1 some edge (b,a) must pass the threshold as well (of duplicates any one suffices).  An edge whose
 *   endpoints lie in different scenes (or out of range) never links and is dropped from the output.
 * Objects = the connected components of the undirected link graph.  root[n] = the lowest node row of n's component; object[n] = the
 *   dense index of that root among all roots in ascending order, so the objects of a scene are contiguous and in scene order.
 *   n_objects[s] = objects of scene s; totals = {M, E'} = objects and merged edges of the batch.
 * Members.  member_ptr int32 [N+1], members int32 [N]: CSR; the members of object o are members[member_ptr[o] .. member_ptr[o+1]) in
 *   ascending node row (the first one is its root).  member_ptr[o] = N for o > M.
 * Pooled node probabilities.  For object o and class c, over the members i in ascending row, starting from 0:
 *   s = fl(s + fl(w_i * p_ic)),  W = fl(W + w_i),  merged_probs[o,c] = fl(s / W) -- fp32, every operation rounded on its own (no fused
 *   multiply-add).  obj_weight[o] = W;  obj_batch_ids[o] = the scene of the object.
 * Merged edges.  An input edge with object[a] != object[b] maps to the ordered pair (object[a], object[b]); an edge inside one object,
 *   a self loop and a dropped edge map to -1.  Unique pairs are numbered in the order of their lowest contributing input edge row (no
 *   global sort; a source-major list stays source-major, a list grouped by scene stays grouped).  edge_to_pair int32 [E]; pair_edges
 *   int64 [E,2]; pair_count int32 [E] = input edges folded into the pair; pair_probs f32 [E,R] = the maximum over the contributing
 *   edges, column same_part included (a maximum does not depend on order: exact).
 * Rows past M / E' hold zero; index tables (root is full; members is full; obj_batch_ids, pair_edges, edge_to_pair) hold -1.  Every
 *   field of every output is written by the call.
 * Determinism: the result does not depend on scheduling -- the minimum row defines roots and pair order, the maximum the pair
 *   probabilities, the member order the sums.
 * Limits: n_obj_class 1..1024, n_rel_class 1..32, n_edges <= 2^26, n_edges * n_rel_class < 2^31, n_nodes * n_obj_class < 2^31;
 *   n_scenes > 1 needs batch_ids; anything else is VLSAT_EINVAL, never a clamp.  scratch: vlsat_merge_segments_scratch_bytes(...) bytes,
 *   16-byte aligned (0 = arguments out of range): an open-addressing table of 64-bit keys with the power of two >= 2 n_edges slots
 *   (12 bytes per slot) and 12 bytes per node + 4 per edge + 8 per max(node, edge).  All device pointers; asynchronous on `stream`: no
 *   host synchronisation, no allocation, no runtime fill; integer vector atomics and plain stores only. */
size_t vlsat_merge_segments_scratch_bytes(int64_t n_nodes, int64_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t n_scenes);
int vlsat_merge_segments(const float* obj_probs, const float* rel_probs, const int64_t* edges, const int64_t* batch_ids, const float* weights,
                         int32_t n_nodes, int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t n_scenes, int32_t same_part,
                         float threshold, int32_t mutual, void* scratch, int32_t* root /* [N] */, int32_t* object /* [N] */,
                         int32_t* n_objects /* [n_scenes] */, int32_t* totals /* [2] */, int32_t* member_ptr /* [N+1] */,
                         int32_t* members /* [N] */, float* merged_probs /* [N,C] */, float* obj_weight /* [N] */,
                         int64_t* obj_batch_ids /* [N] */, int32_t* edge_to_pair /* [E] */, int64_t* pair_edges /* [E,2] */,
                         int32_t* pair_count /* [E] */, float* pair_probs /* [E,R] */, void* stream);

/* -------- eval ranking step (the caller of the path: process_val, reference SGFN_MMG/model.py:463-472) --- */

/* out[r, :] = softmax(x[r, 0:cols]) -- F.softmax(objs_pred) of evaluate_triplet_topk
 * (reference src/utils/eva_utils_acc.py:144).  out is dense [rows, cols]. */
int vlsat_k_softmax_rows(const float* x, int32_t ld, int32_t rows, int32_t cols, float* out, void* stream);

/* evaluate_topk_object (eva_utils_acc.py:27-39), evaluate_topk_predicate (:42-79) and
 * evaluate_triplet_topk (:137-213, multi_rel_outputs=True, use_clip=True) as counting kernels; all
 * device pointers.  gt_rel is the multi-hot [E,R] int64 target, edges is [E,2] (from, to) int64 like
 * the `edge_indices` the reference passes.  Outputs: obj_rank [N]; rel_rank / tri_rank [E,R] hold, for
 * edge e, its cnt[e] = max(#gt relations, 1) ranks already sorted and position-adjusted as the reference
 * appends them (first cnt[e] slots, rest 0).  Flattening the used slots in edge order gives exactly
 * the reference's result arrays.  Triplet ranks are counted along a staircase over each node's sorted class probabilities
 * (csrc/eval_ranks.hip): `scratch` holds vlsat_eval_ranks_scratch_floats(n_nodes, n_obj_class, topk_triplet) floats of device
 * memory the call may overwrite (the topk largest probabilities per node; required when n_edges > 0).
 * Precondition: tri_rank is valid only for NON-NEGATIVE rel_probs (and obj_probs) -- the staircase relies on fl(fl(s * o) * r) being
 * monotone in s and o, which a negative r reverses; obj_rank, rel_rank and cnt hold for any finite values.  A single-label model
 * (MODEL.multi_rel_outputs = false: rel_probs are log-probabilities, all <= 0) therefore calls twice: with the raw values for
 * rel_rank -- the reference ranks them as they are, the `threshold` compare of an edge without gt relation included -- and with
 * their exp (vlsat_k_exp) for tri_rank; the tri_rank of the first call and the rel_rank of the second are to be discarded.
 * vlsat_process_val_counts does both in one pass. */
int vlsat_eval_ranks(const float* obj_logits, const float* obj_probs, const float* rel_probs,
                     const int64_t* gt_class, const int64_t* gt_rel, const int64_t* edges,
                     int32_t n_nodes, int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class,
                     int32_t topk_obj, int32_t topk_rel, int32_t topk_triplet, float threshold,
                     int32_t* obj_rank, int32_t* rel_rank, int32_t* tri_rank, int32_t* cnt, float* scratch, void* stream);
int64_t vlsat_eval_ranks_scratch_floats(int32_t n_nodes, int32_t n_obj_class, int32_t topk_triplet);

/* Rank arrays of one batch (the outputs of two vlsat_eval_ranks calls, 3D and 2D; cnt is the same for both: it depends on
 * the labels only) -> the ADDITIVE counts MMGNet.validation's summaries are functions of (reference src/model/model.py:
 * 214-242,267-282,364-388; get_mean_recall eva_utils_acc.py:224-237): counts[i] += ... for the 1 + R + 2 (11 + 6 R) = 361
 * fields of cvpr2023-vlsat_amd/evaluate.py fields() (scenes | cm_ge{1..R} | per branch: obj_n, obj_hit@{1,5,10}, rel_n,
 * rel_hit@{1,3,5}, tri_n, tri_hit@{50,100}, per predicate class n, tri@{50,100}, rel@{1,3,5}); obj_topk of the cls_matrix is the
 * 3D object rank for both branches (SGFN_MMG/model.py:469-470).  counts: device uint64, zeroed by the caller before the first
 * scene; integer atomics only, so scenes may be accumulated from several streams at once and the sums are exact.  This is
 * what lets a one-scene-per-call evaluation loop (validation()'s batch_size = 1, src/model/model.py:185) run without a host
 * round trip per scene.  All device pointers; asynchronous.
 * 3D-only: obj_rank_2d, rel_rank_2d and tri_rank_2d all NULL counts the 3D branch alone -- scenes, cm_ge* and the 3D block get exactly
 * what the two-branch call adds, the 2D block of counts is NOT TOUCHED (the vector is additive: a caller may mix both kinds of
 * batch).  The three go together: some NULL and some not is VLSAT_EINVAL before any launch (a table without rows -- n_nodes = 0
 * for obj_rank_2d, n_edges = 0 for the other two -- is not looked at, as before). */
int vlsat_eval_counts(const int32_t* obj_rank_3d, const int32_t* obj_rank_2d, const int32_t* rel_rank_3d, const int32_t* rel_rank_2d,
                      const int32_t* tri_rank_3d, const int32_t* tri_rank_2d, const int32_t* cnt, const int64_t* gt_class,
                      const int64_t* gt_rel, const int64_t* edges, int32_t n_nodes, int32_t n_edges, int32_t n_rel_class,
                      int32_t n_scenes, uint64_t* counts, void* stream);

/* Zero-shot split of the triplet recall: the counts behind get_zero_shot_recall (reference src/utils/eva_utils_acc.py:267-333,
 * called by MMGNet.validation at src/model/model.py:253), for both branches.
 *   rows     the cls_matrix rows that carry a predicate (the -1 "no relation" rows are not counted, unlike vlsat_eval_counts'
 *            tri_n): slot j of edge e is its j-th gt predicate in ascending class order (gt_rel[e, p] == 1), with key
 *            (gt_class[edges[e, 0]], gt_class[edges[e, 1]], p) and ranks tri_rank_{3d,2d}[e * n_rel_class + j] -- the layout
 *            vlsat_eval_ranks writes (cnt as it writes it).
 *   table    uint8 [n_obj_class * n_obj_class * n_rel_class]; table[(s * n_obj_class + o) * n_rel_class + p] = 1 marks a
 *            zero-shot key: one that occurs in the validation annotations and never in the training annotations
 *            (cvpr2023-vlsat_amd/zeroshot.py zero_shot_table; 665 600 bytes for 160 x 160 x 26).  A row whose subject or
 *            object class lies outside [0, n_obj_class) is non-zero-shot; the table is then not read.
 *   counts   uint64 [12], counts[i] += ...: for the 3D and then the 2D ranks, all_n, all_hit@50, all_hit@100, zs_n, zs_hit@50,
 *            zs_hit@100 (hit@K: rank <= K).  Non-zero-shot = all - zs.  Recall = hit / n * 100; an empty group is NaN.
 * n_rel_class <= 32 (as vlsat_eval_counts).  Zeroed by the caller before the first scene; integer atomics only, so scenes may be
 * accumulated from several streams.  All device pointers; asynchronous: no host synchronisation, no runtime fill.
 * 3D-only: tri_rank_2d NULL counts the 3D half (counts[0..5]) alone; counts[6..11] are not touched. */
int vlsat_eval_triplet_split(const int32_t* tri_rank_3d, const int32_t* tri_rank_2d, const int32_t* cnt, const int64_t* gt_class,
                             const int64_t* gt_rel, const int64_t* edges, const uint8_t* table, int32_t n_edges, int32_t n_obj_class,
                             int32_t n_rel_class, uint64_t* counts, void* stream);

/* Scene-graph Recall@K and mR@K: the counts behind evaluate_triplet_recallk / evaluate_triplet_mrecallk (reference
 * src/utils/eval_utils_recall.py, called per scene by process_val2 / process_val3, SGFN_MMG/model_in21k.py:439-500) for
 * the four variants PredCls GC / NGC (evaluate='rels', topk_each = 1 / 100) and SGCls GC / NGC (evaluate='triplet'),
 * at K = 20, 50, 100, for every scene of a batch in one call (csrc/eval_recall.hip).
 *   scores   SGCls conf(e,i,j,k) = fl(fl(s_i * o_j) * r_k) (no FMA), s / o = obj_probs[from] / obj_probs[to] (the softmax of
 *            the logits: use_clip=True); PredCls conf(e,k) = r_k; r = rel_probs[e] -- pass exp(log-probabilities) when the
 *            model has multi_rel_outputs = false.  gt_rel is the multi-hot [E, R] int64 target (get_gt's predicate set).
 *   hit      edge e hits at K when some correct entry c (sub class gt_class[from], obj class gt_class[to], predicate in the
 *            gt set; PredCls: the predicate only) is one of e's min(topk_each, #entries) largest entries and fewer than K
 *            candidates of its scene are STRICTLY greater than c.  Ties at the K boundary therefore resolve optimistically
 *            (the reference's order among equal scores is torch.topk's); whenever the boundary values differ the counts
 *            are the reference's.
 *   counts   int64 [n_scenes][F], F = 1 + R + 4 (3 + 3 R), every field written (no zeroing needed):
 *            gt_edges (edges with >= 1 gt predicate), gt_per_class[R], then for predcls_gc, predcls_ngc, sgcls_gc,
 *            sgcls_ngc in this order: hit@{20,50,100}, class_hit@20[R], class_hit@50[R], class_hit@100[R] (a hit edge adds
 *            1 to every class of its gt set, as evaluate_triplet_mrecallk does).  Recall@K = hit@K / gt_edges.
 *            Variants whose bit (1, 2, 4, 8 in that order) is clear in variants_mask are written as zeros and cost nothing.
 * Preconditions: the scene of edge e is batch_ids[edges[e, 0]] in [0, n_scenes) (batch_ids may be NULL for one scene), and
 * edges arrive grouped by scene in ascending scene order (collate_fn_mmg, evaluate.merge_batches); node and class indices
 * are in range; no NaN.  n_obj_class <= 1024, n_rel_class <= 32.  scratch: vlsat_eval_recallk_scratch_bytes(...) bytes of
 * device memory the call may overwrite (about 4 (N x min(C, 100) + E x (R + 104)) bytes: 50.5 MiB for the 64-scene,
 * 99 840-edge batch, 19.8 MiB for one 39 800-edge scene).  All device pointers;
 * asynchronous on `stream`: no host synchronisation, no runtime fill. */
int vlsat_eval_recallk(const float* obj_probs, const float* rel_probs, const int64_t* gt_class, const int64_t* gt_rel,
                       const int64_t* edges, const int64_t* batch_ids, int32_t n_nodes, int32_t n_edges, int32_t n_obj_class,
                       int32_t n_rel_class, int32_t n_scenes, int32_t variants_mask, void* scratch, int64_t* counts, void* stream);
int64_t vlsat_eval_recallk_scratch_bytes(int64_t n_nodes, int64_t n_edges, int32_t n_obj_class, int32_t n_rel_class,
                                         int32_t n_scenes);

/* One scene (or batch) of an evaluation loop in ONE call: vlsat_forward + softmax of the object logits + vlsat_eval_ranks for both
 * branches + vlsat_eval_counts, enqueued back to back on `stream` with every intermediate in the plan's own scratch -- what
 * Mmgnet.process_val (reference src/model/SGFN_MMG/model.py:458-480) computes per scene, reduced to what MMGNet.validation keeps of
 * it (src/model/model.py:201-242).  Top-k bounds 11 / 6 / 101 and threshold 0.5 are process_val's.  gt_rel is the multi-hot
 * [E, R] int64 target, edges_e2 the [E, 2] int64 (from, to) list in the plan's edge order, counts as for vlsat_eval_counts.
 * All device pointers; asynchronous; one library call per scene on the host side.
 * Single-label handles (MODEL.multi_rel_outputs = false) take the same call: gt_rel is then the one-hot row of the edge's label
 * with column 0 ("none") cleared (get_gt, eva_utils_acc.py:19-22), the predicate ranks are taken on the log-probabilities as they
 * are and the triplet ranks on their exp (eva_utils_acc.py:146-147), which the triplet kernel applies on load with the function of
 * vlsat_k_exp: the counts are those of vlsat_eval_ranks on the outputs and on vlsat_k_exp of them, in ONE ranking pass per branch,
 * without an [E, R] temporary and in the same scratch.
 * 3D-only: obj_2d_feats NULL runs vlsat_forward without its 2D outputs, ONE softmax, ONE ranking pass and the one-branch counts,
 * all on `stream`, intermediates in the same scratch (the plan's workspace_bytes does not change); the 2D block of counts is not
 * touched.  Both settings of MODEL.multi_rel_outputs take either form. */
int vlsat_process_val_counts(vlsat_handle h, vlsat_plan plan, const float* obj_points, const float* obj_2d_feats,
                             const float* descriptor, const int64_t* gt_class, const int64_t* gt_rel, const int64_t* edges_e2,
                             int32_t n_scenes, uint64_t* counts, void* stream);

/* vlsat_process_val_counts, then vlsat_eval_triplet_split on the triplet ranks it left in the plan's scratch: split_table is the
 * uint8 [C * C * R] zero-shot table of the model's n_obj_class C and n_rel_class R (layout: vlsat_eval_triplet_split),
 * split_counts the device uint64 [12] it accumulates into.  A one-scene-per-call loop with the zero-shot split on stays one
 * library call per scene.  counts and every other argument as for vlsat_process_val_counts; with obj_2d_feats NULL the split is
 * the one-branch one as well (split_counts[6..11] are not touched).  Single-label handles as for vlsat_process_val_counts. */
int vlsat_process_val_counts_split(vlsat_handle h, vlsat_plan plan, const float* obj_points, const float* obj_2d_feats,
                                   const float* descriptor, const int64_t* gt_class, const int64_t* gt_rel, const int64_t* edges_e2,
                                   int32_t n_scenes, uint64_t* counts, const uint8_t* split_table, uint64_t* split_counts,
                                   void* stream);

/* The predicted scene graph: for every scene of a batch its top_k (subject, predicate, object) triplets WITH their indices -- the
 * list pred_triplets = ((from, to), (sub cls, obj cls, rel), conf) the reference builds inside evaluate_triplet_recallk
 * (src/utils/eval_utils_recall.py:24-60, 75-96) from its running global top-K and never returns.  No labels are read
 * (csrc/scene_graph.hip).
 *   scores      mode 0 (evaluate='triplet'): conf(e; i, j, k) = fl(fl(s_i * o_j) * r_k) (no FMA), s / o = obj_probs[from] /
 *               obj_probs[to], r = rel_probs[e] -- pass exp(log-probabilities) when the model has multi_rel_outputs = false.
 *               mode 1 (evaluate='rels'): conf(e; k) = r_k; subject and object class are reported as -1; obj_probs is not read.
 *   candidates  per edge its min(topk_each, #entries) largest entries.
 *   output      triplets int32 [n_scenes][top_k][4] = (edge, subject class, object class, predicate), edge being the row of
 *               `edges` (batch-wide: edges[edge] gives the two nodes); scores float [n_scenes][top_k]; n_valid int32 [n_scenes]
 *               = min(top_k, candidates of the scene); rows past n_valid hold -1 / 0.0f.  Every field is written.
 *               1. scores[s, 0:n_valid] is the descending list of the n_valid largest candidate values, bit for bit.
 *               2. a row's score is the product at its (edge, sub, obj, pred); the rows of a scene are pairwise distinct; an
 *                  edge contributes at most topk_each rows.
 *               3. every candidate strictly greater than the last kept score is present.  Which of several candidates EQUAL to
 *                  the last kept score (or to an edge's topk_each-th value) are kept is unspecified (the reference leaves it to
 *                  torch.topk) but a pure function of the scene's own inputs: a batch equals its scenes called one at a time.
 *               4. rows are ordered by score descending, then edge, subject class, object class, predicate ascending.
 *               When the kept values and the first one left out are pairwise different this is the reference's pred_triplets.
 * Limits: top_k 1..1024, topk_each 1..100, n_obj_class <= 1024, n_rel_class <= 32; anything else is an error, never a clamp.
 * Preconditions (as for vlsat_eval_recallk): the scene of edge e is batch_ids[edges[e, 0]] in [0, n_scenes) (batch_ids may be
 * NULL for one scene), edges arrive grouped by scene in ascending scene order, node indices are in range, no NaN, probabilities
 * are non-negative.  scratch: vlsat_scene_graph_scratch_bytes(...) bytes of device memory the call may overwrite
 * (8 (N x min(C, 100) + E x min(topk_each, C C R)) bytes plus the scene offsets; 0 = arguments out of range).  All device
 * pointers; asynchronous on `stream`: no host synchronisation, no runtime fill, no allocation, no global atomics. */
int vlsat_scene_graph_topk(const float* obj_probs, const float* rel_probs, const int64_t* edges, const int64_t* batch_ids,
                           int32_t n_nodes, int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t n_scenes,
                           int32_t mode /* 0 triplet, 1 rels */, int32_t top_k, int32_t topk_each, void* scratch,
                           int32_t* triplets /* [n_scenes][top_k][4]: edge, sub class, obj class, predicate */,
                           float* scores /* [n_scenes][top_k] */, int32_t* n_valid /* [n_scenes] */, void* stream);
int64_t vlsat_scene_graph_scratch_bytes(int64_t n_nodes, int64_t n_edges, int32_t n_obj_class, int32_t n_rel_class,
                                        int32_t n_scenes, int32_t top_k, int32_t topk_each);

/* out[i] = expf(x[i]) for n floats (out may be x): turns the log-probabilities of a MODEL.multi_rel_outputs = false model into
 * the rel_probs of vlsat_scene_graph_topk with the kernel vlsat_forward_scene_graph uses (so the separate calls equal the one
 * call bit for bit).  Device pointers; asynchronous. */
int vlsat_k_exp(const float* x, int64_t n, float* out, void* stream);

/* The label-free sibling of vlsat_process_val_counts: vlsat_forward + softmax of both object heads + vlsat_scene_graph_topk for
 * both branches, enqueued back to back on `stream` with every intermediate in the plan's own memory (the selection's candidate
 * slots re-use an edge tensor that is dead once the forward has finished: the plan's arena does not grow) -- one library call
 * per scene from an unlabelled scan to its predicted graph.  edges_e2 is the [E, 2] int64 (from, to) list in the plan's edge
 * order; n_scenes must be the plan's scene count (the scenes are the plan's).  With MODEL.multi_rel_outputs = false the
 * log-probabilities are exponentiated on the device.  Outputs per branch as for vlsat_scene_graph_topk.  All device pointers;
 * asynchronous.
 * 3D-only: obj_2d_feats and the three 2D outputs go together -- all given, or all NULL: the 3D-only forward and one selection
 * (a single-label model's log-probabilities are still exponentiated in place).  Any mixture is VLSAT_EINVAL before anything is
 * launched; the outputs are then untouched. */
int vlsat_forward_scene_graph(vlsat_handle h, vlsat_plan plan, const float* obj_points, const float* obj_2d_feats,
                              const float* descriptor, const int64_t* edges_e2, int32_t n_scenes, int32_t mode,
                              int32_t top_k, int32_t topk_each, int32_t* triplets_3d, float* scores_3d, int32_t* n_valid_3d,
                              int32_t* triplets_2d, float* scores_2d, int32_t* n_valid_2d, void* stream);

/* The decoded scene graph: one label per object with a few alternatives, and per ordered pair the predicates the model ASSERTS --
 * the decision rule the reference's evaluation states (src/utils/eva_utils_acc.py:42-63, 176-181: a multi-label edge predicts "none"
 * exactly when no predicate reaches confidence_threshold = 0.5; get_gt :19-22: class 0 of a single-label edge is "none") applied
 * to the outputs of every scene of a batch (csrc/graph_decode.hip).  No labels are read.
 *   nodes       labels int32 / label_probs float [n_nodes][n_labels]: the n_labels largest entries of obj_probs[n, :], descending,
 *               equal values in ascending class order.
 *   decisions   multi_label = 1: predicate k of edge e is asserted iff rel_probs[e, k] >= thresholds[k] (fp32 compare; equality
 *               passes).  multi_label = 0: k* = the lowest index of the row maximum; the edge asserts k* iff k* != 0 and
 *               rel_probs[e, k*] >= thresholds[k*] -- pass exp(log-probabilities) of a MODEL.multi_rel_outputs = false model.
 *               thresholds: float [n_rel_class] in DEVICE memory.
 *   score       score_mode 0: rel_probs[e, k].  score_mode 1: fl(fl(s * o) * rel_probs[e, k]) (two roundings, no FMA), s / o the
 *               top-1 probabilities of the edge's two nodes.
 *   output      n_total int32 [n_scenes] = asserted (e, k) pairs of the scene; n_valid = min(n_total, max_rel); rels int32
 *               [n_scenes][max_rel][2] = (edge, predicate), edge being the row of `edges` (batch-wide); scores float
 *               [n_scenes][max_rel]; the rows of a scene are the first n_valid of its asserted pairs under the total order (score
 *               descending, edge ascending, predicate ascending); rows past n_valid hold -1 / 0.0f.  Every field is written, and
 *               the output is fully determined by the inputs: there is no unspecified tie rule.
 * Limits: n_labels 1..8 (and <= n_obj_class), max_rel 1..4096, n_obj_class <= 1024, n_rel_class <= 32, n_edges <= 2^26 and
 * n_edges * n_rel_class < 2^31; anything else is an error, never a clamp.  Preconditions (as for vlsat_scene_graph_topk): the
 * scene of edge e is batch_ids[edges[e, 0]] in [0, n_scenes) (batch_ids may be NULL for one scene), edges arrive grouped by scene
 * in ascending scene order, node indices are in range, no NaN, probabilities are non-negative.  scratch:
 * vlsat_graph_decode_scratch_bytes(...) bytes of device memory the call may overwrite (n_edges x (5 n_rel_class + 4) bytes -- per
 * edge its asserted predicates as sorted 4-byte keys with a 1-byte predicate each, and their number -- plus the scene offsets;
 * 0 = arguments out of range).  All device pointers; asynchronous on `stream`: no host synchronisation, no runtime fill, no
 * allocation, no global atomics. */
int vlsat_graph_decode(const float* obj_probs, const float* rel_probs, const int64_t* edges, const int64_t* batch_ids,
                       const float* thresholds, int32_t n_nodes, int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class,
                       int32_t n_scenes, int32_t multi_label, int32_t score_mode /* 0 rel, 1 triplet */, int32_t n_labels,
                       int32_t max_rel, void* scratch, int32_t* labels /* [n_nodes][n_labels] */,
                       float* label_probs /* [n_nodes][n_labels] */, int32_t* rels /* [n_scenes][max_rel][2]: edge, predicate */,
                       float* scores /* [n_scenes][max_rel] */, int32_t* n_valid /* [n_scenes] */, int32_t* n_total /* [n_scenes] */,
                       void* stream);
int64_t vlsat_graph_decode_scratch_bytes(int64_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t n_scenes,
                                         int32_t n_labels, int32_t max_rel);

/* The decisions of vlsat_graph_decode BEFORE the cap, counted against ground truth: what a user chooses thresholds by.
 * counts uint64 [3 * n_rel_class + 2], counts[i] += ...: per predicate k tp, fp, fn at 3 k + {0, 1, 2} (asserted and in gt,
 * asserted and not in gt, in gt and not asserted), then nodes, then nodes whose top-1 class (lowest index of the row maximum) is
 * gt_class.  gt_rel: multi_label = 1 the int64 multi-hot [n_edges][n_rel_class] vlsat_process_val_counts takes; multi_label = 0
 * int64 [n_edges] with 0 = none (the counts of predicate 0 stay zero).  Zeroed by the caller before the first batch; integer
 * atomics only, so batches may be accumulated from several streams and the sums are exact.  All device pointers; asynchronous. */
int vlsat_graph_decode_counts(const float* obj_probs, const float* rel_probs, const int64_t* gt_class, const int64_t* gt_rel,
                              const float* thresholds, int32_t n_nodes, int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class,
                              int32_t multi_label, uint64_t* counts, void* stream);

/* From points to the decoded graph in ONE call: vlsat_forward + softmax of the object heads (+ exp of the log-probabilities when
 * MODEL.multi_rel_outputs = false) + vlsat_graph_decode per branch, enqueued back to back on `stream` with every intermediate in
 * the plan's own memory (the compaction slots live in the evaluation scratch the plan already owns: the arena does not grow).
 * obj_2d_feats == NULL selects the 3D-only forward (vlsat_forward with NULL 2D arguments): an unlabelled scan has no 2D features,
 * because the reference's feature files are named after the ground-truth class.  Every 2D output pointer must then be NULL too;
 * with obj_2d_feats every output is required; any other mix is VLSAT_EINVAL.  edges_e2 is the [E, 2] int64 (from, to) list in the
 * plan's edge order; n_scenes must be the plan's scene count.  thresholds: device float [n_rel_class].  Outputs per branch as for
 * vlsat_graph_decode.  All device pointers; asynchronous. */
int vlsat_forward_graph(vlsat_handle h, vlsat_plan plan, const float* obj_points, const float* obj_2d_feats, const float* descriptor,
                        const int64_t* edges_e2, int32_t n_scenes, int32_t multi_label, int32_t score_mode, int32_t n_labels,
                        int32_t max_rel, const float* thresholds, int32_t* labels_3d, float* label_probs_3d, int32_t* rels_3d,
                        float* scores_3d, int32_t* n_valid_3d, int32_t* n_total_3d, int32_t* labels_2d, float* label_probs_2d,
                        int32_t* rels_2d, float* scores_2d, int32_t* n_valid_2d, int32_t* n_total_2d, void* stream);

/* The additive fp64 metrics vector of one rank's batch -- what the path's one all-reduce carries when no labels are at hand
 * (bench.py; the label-based counts of validation(), reference src/model/model.py:214-242, come from vlsat_eval_ranks):
 * out9 = {n_scenes, n_nodes, n_edges, sum obj3d, sum obj2d, sum rel3d, sum rel2d, #nodes whose 3D and 2D top-1 class agree,
 * #edges whose 3D and 2D top-1 relation agree}.  All device pointers; the outputs are the dense [n_nodes, n_obj_class] /
 * [n_edges, n_rel_class] tensors vlsat_forward wrote; scratch holds 256 * 6 doubles.  Two launches on `stream`, fixed
 * summation order (no atomics): bit-reproducible. */
int vlsat_scene_checksums(const float* obj3d, const float* obj2d, int64_t n_nodes, int32_t n_obj_class, const float* rel3d,
                          const float* rel2d, int64_t n_edges, int32_t n_rel_class, int32_t n_scenes, double* out9, double* scratch,
                          void* stream);

/* -------- debug / test hooks (used by tests/ to localise a parity failure) -------------------- */
/* Stop vlsat_forward after stage `stage` (-1 = run everything).  Stages: 1 object encoder,
 * 2 node embedding, 3 edge embedding, 4 adapter, 5 distance bias, then for layer l:
 * 10+10l self-attention, +1 cross-attention, +2 gcn_3ds, +3 gcn_2ds, +4 edge cross-attention. */
int vlsat_debug_stop_after(vlsat_handle h, int32_t stage);
/* Device pointer and shape of a named workspace buffer of a plan ("X3","X2","E3","E2","F","G",
 * "AGG3","AGG2","H1","KP","NP","Hbig","bias","On","Oe","Qe","KVe").  "G" (gated values) and "AGG3"/"AGG2" keep
 * their 256 channels head-major (h*32 + m); the reference's order is m*8 + h. */
int vlsat_debug_buffer(vlsat_plan p, const char* name, void** ptr, int64_t* rows, int32_t* cols, int32_t* ld);
/* Synchronous strided device-to-device copy of that buffer into dst (row pitch dst_ld floats). */
int vlsat_debug_read(vlsat_plan p, const char* name, float* dst, int64_t dst_ld);

/* DVFS probe: while buf (device, >= 4*512 int64, zeroed) is non-NULL every block of the persistent GEMM
 * writes {shader cycles (s_memtime), 100 MHz wall ticks (s_memrealtime), tiles done, 1} when it exits;
 * cycles / (ticks / 1e8) is the shader clock the kernel actually ran at. NULL disables. */
int vlsat_debug_gemm_clock_probe(int64_t* buf);

/* Switches of one handle; defaults are the measured-best settings and none changes results beyond fp32 summation order / the
 * precision mode's rounding.  The RELEASE library accepts:
 *   "dual_stream" 0|1|2   extra streams for the 2D chains (1: launch-bound plans only, 2 = default: every plan; such a plan owns a second
 *                         scratch set, +11.3 KB per edge, and falls back to one stream past 48 GiB of workspace) -- plans created afterwards;
 *   "sched" -1|0|1        schedule of a multi-stream plan: 1 = dependency-exact, three lanes (3D chain / 2D edge chain / 2D node chain)
 *                         coupled by one event per data-flow edge; 0 = fork / join, lanes meet twice per layer; -1 (default) = exact on
 *                         plans of more than 16 384 edges (every precision mode), fork / join otherwise.  Bit-identical results;
 *   "flash_split" 0|1     split-key edge attention for plans that cannot fill the chip (plans created afterwards);
 *   "prof_dual" 0|1       per-class profiling keeps the multi-stream execution (1, default) or serialises on the launch stream;
 *   "pair_twins" 0|1, "pair_max_edges" n   plans of at most n edges (default 4096: one scene per call) run the 3D / 2D twin stages --
 *                         relation encoders, gcn_3ds | gcn_2ds, both head pairs -- as launches of two problems each, the edge cross-attention
 *                         of layer l on the second stream under the node attentions of layer l + 1 (round 6).  Bit-identical results;
 *   "gemm_p8", "gemm_dma", "gemm_splitk" 0|1          GEMM kernel selection (0: the older kernels);
 *   "gemm_splitk_max_tiles" n   the split-K kernel takes launches of at most n 64 x 64 output tiles (default 64; 0: half the resident slots);
 *   "gemm_p8_part_min" n   8-phase GEMM: remainder tiles (behind full rounds of 256 x 256 tiles) from which the launch takes them along as one
 *                         more, balanced round instead of leaving them to a tail launch; 0 = default by precision: 12 single-rounding bf16,
 *                         24 split-bf16, 5/8 of a round exact fp32 (profiles/r06_probes/ab_p8_part_min_*.txt);
 *   "gemm_k_rot" -1|0..7  8-phase GEMM: column tile tn of a row panel walks its K-tiles starting at tn * r (the blocks that share an A
 *                         panel ask L2 for its lines out of step); -1 = default: 1 for half-row bf16 launches, 0 otherwise.  Rotates an
 *                         fp32 summation order: inside every mode's tolerance (tests/test_hip_round6.py), not bit-identical;
 *   "gather_f16" -1|0|1   the node-side tables [P_i | P_j] that nn_edge.0 adds per edge (reference network_MMG.py:59-60,92: cat[x_i, e, x_j] as
 *                         three partial products) as fp16 half rows instead of fp32: half the gathered bytes, 2^-12 relative rounding of two
 *                         summands in front of a ReLU whose output is rounded to bf16 anyway; -1 = default: on in the single-rounding modes
 *                         (bf16_mixed, bf16), off in the split-bf16 ones, never in fp32;
 *   "outproj_f16" -1|0|1  the out-projection of a single-rounded edge attention (bf16_mixed, bf16, bf16x3_attn1) hands its rows to the
 *                         LayerNorm as fp16 half rows instead of fp32 (-1 = default: on);
 *   "split_fmt", "flash_bf16", "flash_tr", "pointnet_bf16", "gate_bf16", "ln_resid" 0|1   bf16 modes: tensor formats and kernels (0: the
 *                         fp32 forms) -- every one parity-tested both ways (tests/test_hip_forward.py);
 *   "flash_exact" -1|0|1  fp32 mode at head dim 64: the edge cross-attention's products as three fp16 MFMAs each (-1 = default, 0), or the
 *                         exact fp32-MFMA kernel (1): the forward of the releases before the split-fp16 kernel, bit for bit, without its
 *                         operand domain (|Q / sqrt(d_k) * log2 e|, |K| < 65504, |V| < 8188);
 *   "gemm_exact" -1|0|1   fp32 mode: the full rounds of the large edge-row GEMM launches as three fp16 MFMAs per product (-1 = default, 0), or
 *                         on the exact fp32-MFMA kernel (1), without the operand domain |A| <= 65504; with "flash_exact" 1: the forward of
 *                         the releases before either split-fp16 kernel, bit for bit;
 *   "flash_bq_big" 0|1    half-row edge attention, plans whose scenes all have >= 4096 edges: 256 queries per block (default) or 128;
 *   "flash_bq_big_min" n  ... that bound (plans created afterwards).  At the bench batch (1560 edges per scene) 256-query tiles are 1 %
 *                         slower per step than 128-query ones (profiles/r06_probes/ab_flash_bq_big_min.txt): the default stays 4096;
 *   "flash_qg" 0|1|2      half-row edge attention at head dim 64, no key split: 64 queries per wave (two 32-query groups share every K / V
 *                         fragment; 2 = group 0's P.V product in front of group 1's softmax).  Bit-identical to 0; 4-7 % slower per step
 *                         at BASELINE configs[2] and configs[4] (profiles/r06_probes/ab_flash_qg.txt): default 0;
 *   "flash_pv_terms" 3|2  split-bf16 edge attention: MFMAs per P.V product;  "gate_fuse_agg" 0|1|2: max aggregation inside the gate
 *                         kernel (never / default: bf16 modes, and fp32 on plans of more than 16 384 edges / fp32 on every plan);
 *                         "gate_row_map" 0|1, "gate_heads_mfma" 0|1|2: gate kernel variants; "gate_exact" -1|0|1: fp32 mode, the edge
 *                         gate of 8 heads x (64, 32) as three fp16 MFMAs per product (-1, 0) or on the exact fp32-MFMA kernel (1);
 *   "edge_pairs", "edge_pairs_e2" 0|1   fp32 mode: edge tensors between the split-fp16 kernels as pair words (csrc/edge_pairs.h; default 1),
 *                         the second one for the 2D chain tensor E2 as the LayerNorm and rel_encoder_2d write it.  Bit-identical results.
 * Lab switches ("gate_grid", "gate_heads_bf16", "flash_heads_bf16", "node_attn_split", "half_fmt", "flash_dma", "flash_ablate" -- the
 * last one produces GARBAGE results for timing) exist in the experiments build only (`build.py --experiments`, -DVLSAT_EXPERIMENTS ->
 * tools/bin/libvlsat_hip_exp.so); the release library answers them with VLSAT_EINVAL. */
int vlsat_debug_option(vlsat_handle h, const char* name, int32_t value);

/* ---- the one collective of the path: sum of a short fp64 metrics vector over ranks, on RCCL ---------------
 * Scenes are sharded over ranks with no data-path exchange; a sharded evaluation ends with one all-reduce of additive
 * counts (what the reference's validation() computes its percentages from, src/model/model.py:214-242).  RCCL is
 * resolved at run time (the copy already in the process, e.g. PyTorch's, else librccl.so.1): no link-time dependency.
 * Bootstrap: rank 0 calls vlsat_comm_unique_id (128 bytes), the host shares them with the other ranks (file, pipe,
 * any launcher), every rank calls vlsat_comm_init with its GPU current. */
int vlsat_comm_unique_id(void* out128);
int vlsat_comm_init(const void* id128, int32_t n_ranks, int32_t rank, void** comm);
/* buf: device fp64[n], summed over ranks in place; asynchronous on `stream`. */
int vlsat_metrics_allreduce(void* comm, double* buf, int32_t n, void* stream);
void vlsat_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* VLSAT_H */
