// The interface between binding.cpp and the HIP kernels: every GPU launcher is declared here
// once, and so is every list of compiled tile variants of the decode-GEMM family.
//
// binding.cpp (host g++) and the .hip file that defines a launcher (hipcc) both include this
// header, so a signature that differs between the two is a compile error instead of a wrong
// stride or a wild pointer at run time.  The contract of each launcher (shapes, alignment,
// what it refuses) is the comment on its definition.  The host AdamW has its own header,
// cpu/cpu_adam.h: that file is compiled without the ROCm include path.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

// ---- compiled tile variants of the decode GEMMs ---------------------------------------------------
// Each X-macro is expanded by its kernel file into the launch dispatch and by binding.cpp into
// the argument check and _C.variants(); lumen/ops/gemm.py keeps literal tables for machines
// without the extension and tests/test_kernels_gpu.py compares them with _C.variants().

// decode_gemm.hip: X(BM, BN, WM, WN), WM x WN waves.  4 waves: BM 256 -> 4 x 1, 128 -> 2 x 2,
// 64 -> 1 x 4; 8 waves: BM 256 -> 4 x 2, 128 -> 2 x 4
#define LUMEN_DG_VARIANTS(X)                                                                   \
  X(256, 64, 4, 1) X(256, 96, 4, 1) X(256, 128, 4, 1) X(256, 160, 4, 1)                         \
  X(192, 64, 4, 1) X(192, 96, 4, 1) X(192, 128, 4, 1)                                           \
  X(128, 64, 2, 2) X(128, 96, 2, 2) X(128, 128, 2, 2) X(128, 192, 2, 2) X(128, 256, 2, 2)       \
  X(64, 64, 1, 4) X(64, 128, 1, 4) X(64, 192, 1, 4) X(64, 256, 1, 4)                            \
  X(256, 64, 4, 2) X(256, 128, 4, 2) X(128, 128, 2, 4) X(128, 256, 2, 4)

// k-tiled x variants (flags bit 1): the BM = 256 tiles
#define LUMEN_DG_XT_VARIANTS(X) X(256, 64, 4, 1) X(256, 128, 4, 1) X(256, 64, 4, 2) X(256, 128, 4, 2)

// the quantized families: X(BM, BN), 4 waves each
#define LUMEN_W8_VARIANTS(X) X(64, 64) X(64, 128) X(128, 64) X(128, 128) X(256, 64)

#define LUMEN_W8A8_VARIANTS(X) \
  X(64, 64) X(64, 128) X(128, 64) X(128, 128) X(128, 256) X(256, 64) X(256, 128)

#define LUMEN_W4A8_VARIANTS(X) \
  X(16, 64) X(16, 128) X(64, 64) X(64, 128) X(128, 64) X(128, 128) X(256, 64)

#define LUMEN_W4A16_VARIANTS(X) X(64, 64) X(64, 128) X(128, 64) X(128, 128) X(256, 64)

// ---- launchers, by the file that defines them -----------------------------------------------------
extern "C" {

// adamw.hip
hipError_t lumen_grad_norm_sq(int gdtype, const void* g, long long n, float* out, hipStream_t st);
hipError_t lumen_adamw(float* p, int gdtype, const void* g, float* m, float* v, int out_dtype,
                       void* out_copy, long long n, float lr, float beta1, float beta2, float eps,
                       float wd, float bc1, float bc2, float inv_scale, const float* norm_sq,
                       float max_norm, float* step_state, const double* sched, hipStream_t st);

// calib.hip
hipError_t lumen_hbm_read(const void* p, long long bytes, unsigned* out, int blocks,
                          hipStream_t st);

// cross_entropy.hip
hipError_t lumen_scale_dev(int dtype, void* x, long long n, const float* num, const float* den,
                           hipStream_t st);
hipError_t lumen_cross_entropy(int dtype, void* logits, const int64_t* labels, float* loss_sum,
                               float* row_loss, int rows, int V, int ignore_index, float scale,
                               int write_grad, const float* gscale, hipStream_t st);

// custom_ar.hip
long long lumen_car_signal_bytes();
int lumen_car_max_blocks();
int lumen_car_max_ranks();
hipError_t lumen_car_alloc(long long bytes, int cached, void** ptr);
hipError_t lumen_car_free(void* ptr);
hipError_t lumen_car_get_handle(void* ptr, void* handle_out /* hipIpcMemHandle_t bytes */);
int lumen_car_handle_bytes();
hipError_t lumen_car_open_handle(const void* handle, void** ptr);
hipError_t lumen_car_close_handle(void* ptr);
hipError_t lumen_car_host_flag_alloc(void** host, void** dev);
hipError_t lumen_car_host_flag_free(void* host);
hipError_t lumen_car_read_err(void* sig, unsigned int* err);
hipError_t lumen_car_read_diag(void* sig, unsigned int* out);
hipError_t lumen_car_allreduce(int dtype, const long long* data, const long long* sig, int rank,
                               int world, const void* in, void* out, long long numel, int two_shot,
                               int blocks, double timeout_s, void* host_err, hipStream_t st);
hipError_t lumen_car_allgather(int dtype, const long long* data, const long long* sig, int rank,
                               int world, const void* in, void* out, long long rows,
                               long long shard_cols, int blocks, double timeout_s, void* host_err,
                               hipStream_t st);

// decode_gemm.hip
hipError_t lumen_decode_gemm(int dtype, const void* x, const void* W, void* y, float* ws, int* cnt,
                             int M, int N, int K, long long ldx, long long ldy, int BM, int BN,
                             int NW, int S, int flags, hipStream_t st);

// embedding.hip
hipError_t lumen_embedding(const void* W, const long long* ids, void* out, int T, int V, int H,
                           hipStream_t st);

// flash_attn.hip
hipError_t lumen_flash_attn(int dtype, int which, int causal, int mt, const void* q, const void* k,
                            const void* v, long long ldq, long long ldk, long long ldv, void* o,
                            long long ldo, float* lse, const int* cu, const int* tiles, int ntiles,
                            int nh, int nkv, int T, float scale, const void* dout, long long lddo,
                            void* dq, void* dk, void* dv, long long lddq, long long lddk,
                            long long lddv, const float* delta, const int* rope_pos,
                            const float* rope_cos, const float* rope_sin, hipStream_t st);
hipError_t lumen_flash_attn_paged(int dtype, int causal, const void* q, long long ldq,
                                  const void* k_cache, const void* v_cache, void* o, long long ldo,
                                  const int* cu_q, const int* kv_lens, const int* tiles, int ntiles,
                                  const int* block_tables, int bt_stride, int block_size, int nh,
                                  int nkv, int T, float scale, hipStream_t st);
hipError_t lumen_flash_attn_ds(int dtype, int which, int causal, const void* q, const void* k,
                               const void* v, long long ldq, long long ldk, long long ldv,
                               const float* lse, const int* cu, const int* tiles, int ntiles,
                               int nh, int nkv, int T, float scale, const void* dout,
                               long long lddo, void* dq, void* dk, void* dv, long long lddq,
                               long long lddk, long long lddv, const float* delta,
                               const int* rope_pos, const float* rope_cos, const float* rope_sin,
                               void* ds, const int* ds_off, int ds_total, hipStream_t st);

// lora.hip
hipError_t lumen_lora_gemm(int act_dtype, int mode, int bn, const void* X, const void* W, void* C,
                           long long ldx, long long ldw, long long cs_m, long long cs_n,
                           float alpha, int ksplit, unsigned long long seed,
                           unsigned int drop_thresh, float drop_scale, long long drop_ld, int nseg,
                           const long long* x_off, const long long* w_off, const long long* c_off,
                           const int* Ms, const int* Ns, const int* Ks, hipStream_t st);

// lora_v2.hip
hipError_t lumen_lora2(int dtype, int kind, int flag, const void* big, long long ldb,
                       const float* small, long long lds, void* out, long long cs0, long long cs1,
                       float alpha, int T, int J, int split, unsigned long long seed,
                       unsigned int drop_thresh, float drop_scale, long long drop_ld,
                       long long drop_col0, int nseg, const long long* big_off,
                       const long long* small_off, const long long* out_off, const int* ncols,
                       const float* rope_cos, const float* rope_sin, const int* rope_pos,
                       int rope_mask, hipStream_t st);

// lora_v3.hip
hipError_t lumen_lora3_w_tail_batch(int dtype, const long long* desc, int n, long long max_chunks,
                                    hipStream_t st);
hipError_t lumen_lora3_down(int dtype, const void* x, long long ldx, const float* A, long long lda,
                            float* Z, long long ldz, int T, int K, int R, float alpha,
                            unsigned long long seed, unsigned int thresh, float drop_scale,
                            long long drop_ld, long long drop_col0, void* xe, long long ldxe,
                            int xk, int KP, unsigned* cnt, float* slab, hipStream_t st);
hipError_t lumen_lora3_up(int dtype, int fwd, void* out, long long ldo, const float* s1,
                          long long ld1, const float* s2, long long ld2, int T, int J, float alpha,
                          unsigned long long seed, unsigned int thresh, float drop_scale,
                          long long drop_ld, long long drop_col0, int nseg,
                          const long long* out_off, const long long* s1_off,
                          const long long* s2_off, const int* ncols, const float* rope_cos,
                          const float* rope_sin, const int* rope_pos, int rope_mask,
                          hipStream_t st);
hipError_t lumen_lora3_dy(int dtype, const void* dy, long long ldy, const float* B, int r,
                          const float* Z, long long ldz, float* dZ, long long lddz, float* dB,
                          int T, int tw, float alpha, int nseg, const long long* n_off,
                          const long long* r_off, const long long* b_off, const int* n_len,
                          float* slab_z, float* slab_b, unsigned* cnt_z, unsigned* cnt_b,
                          hipStream_t st);
hipError_t lumen_lora3_z_tail(int dtype, const float* Z, int R, void* xe, long long ldx, int K,
                              int KP, int T, hipStream_t st);
hipError_t lumen_lora3_w_tail(int dtype, void* w, long long ldw, int K, const float* B, int r,
                              int nseg, const long long* n_off, const long long* b_off,
                              const int* n_len, const int* r_off, float scale, hipStream_t st);
hipError_t lumen_lora3_dxa(int dtype, const void* x, long long ldx, void* dx, long long lddx,
                           const float* dZ, const float* A, long long lda, float* dA,
                           long long ldda, int T, int K, int R, int tw, unsigned long long seed,
                           unsigned int thresh, float drop_scale, long long drop_ld,
                           long long drop_col0, float* delta, float* slab, unsigned* cnt,
                           hipStream_t st);

// mlp_gemm.hip
int lumen_mlp_gemm_split(int M, int N, int K, int epi, int cus);
hipError_t lumen_mlp_gemm(int dtype, int epi, const void* x, long long ldx, const void* w,
                          long long ldw, void* c, long long ldc, void* act, long long ldact,
                          const void* gu, long long ldgu, int M, int N, int K, int F, int group_m,
                          float* ws, int* cnt, int split, hipStream_t st);

// paged_attention.hip
hipError_t lumen_paged_attention_decode(int dtype, void* out, const void* q, const void* kc,
                                        const void* vc, const int* block_tables,
                                        const int* context_lens, int nseq, int nh, int nkv, int D,
                                        int BS, int max_blocks, int max_parts, float scale,
                                        float* tmp_m, float* tmp_l, void* tmp_o, int PART,
                                        unsigned* counters, int one_pass, int fp8kv, int qldh,
                                        hipStream_t st);
hipError_t lumen_reshape_and_cache(int dtype, const void* k, const void* v, void* kc, void* vc,
                                   const long long* slots, int ntok, int nkv, int D, int BS,
                                   long long k_stride, long long v_stride, int fp8kv,
                                   hipStream_t st);
hipError_t lumen_rope_cache(int dtype, void* qkv, long long ld, const int* pos, const float* cos_t,
                            const float* sin_t, void* kc, void* vc, const long long* slots,
                            int ntok, int nh, int nkv, int D, int BS, int fp8kv, hipStream_t st);
hipError_t lumen_kv_dequant(int dtype, const void* kc, const void* vc, void* ks, void* vs,
                            const int* tables, int tstride, const int* kv_lens, int nseq, int maxb,
                            int nkv, int BS, int D, hipStream_t st);
hipError_t lumen_kv_dequant_mx(int dtype, const void* kc, const void* vc, void* ks, void* vs,
                               const int* tables, int tstride, const int* kv_lens, int nseq,
                               int maxb, int nkv, int BS, int D, hipStream_t st);

// qbase.hip
hipError_t lumen_qbase_dequant(int fmt, int dtype, const void* q, const void* scale, void* out,
                               long long N, long long K, long long ld, hipStream_t st);
hipError_t lumen_qbase_dequant_t(int fmt, int dtype, const void* q, const void* scale, void* out,
                                 long long N, long long K, hipStream_t st);

// rmsnorm.hip
void lumen_set_rms_lds(int fwd_bytes, int bwd_bytes);
hipError_t lumen_rmsnorm_fwd_ld(int dtype, const void* x, const void* residual, const void* w,
                                void* y, void* s_out, float* rstd, int rows, int H, float eps,
                                long long ldy, hipStream_t st);
hipError_t lumen_rmsnorm_fwd(int dtype, const void* x, const void* residual, const void* w, void* y,
                             void* s_out, float* rstd, int rows, int H, float eps, hipStream_t st);
hipError_t lumen_rmsnorm_bwd(int dtype, const void* dy, const void* s, const void* w,
                             const float* rstd, const void* ds_res, void* dx, float* dw, int rows,
                             int H, hipStream_t st);

// rope.hip
hipError_t lumen_qkv_rope(int dtype, int bwd, void* qkv, void* q, void* k, void* v, const int* pos,
                          const float* cos_t, const float* sin_t, int T_tokens, int S, int nh,
                          int nkv, int D, hipStream_t st);
hipError_t lumen_rope_inplace(int dtype, void* x, const int* pos, const float* cos_t,
                              const float* sin_t, int T_tokens, int row_stride, int nheads, int D,
                              hipStream_t st);

// sampling.hip
hipError_t lumen_sample(int dtype, const void* logits, const float* temperature, const float* top_p,
                        const int* top_k, unsigned long long seed, long long offset,
                        long long* out_tok, float* out_lp, float* out_tau, int rows, int V,
                        hipStream_t st);

// sampling_rows.hip
hipError_t lumen_sample_rows(int dtype, const void* logits, const float* temperature,
                             const float* top_p, const int* top_k, const long long* seed,
                             const long long* offset, const long long* rngrow, const float* min_p,
                             const int* bias_ptr, const int* bias_idx, const float* bias_val,
                             const int* slot, const float* rp, const float* fp, const float* pp,
                             int* counts, int S, int pre, const long long* g_table,
                             const int* g_slot, int* g_state, int G, long long* out_tok,
                             float* out_lp, float* out_tau, int rows, int V, hipStream_t st);
hipError_t lumen_logits_process(int dtype, const void* logits, const int* bias_ptr,
                                const int* bias_idx, const float* bias_val, const int* slot,
                                const float* rp, const float* fp, const float* pp,
                                const int* counts, int S, const long long* g_table,
                                const int* g_slot, const int* g_state, int G, float* out,
                                int rows, int V, hipStream_t st);
hipError_t lumen_sampler_state_init(int* counts, const int* slots, const int* ptr,
                                    const int* n_prompt, const int* ids, int n, int S, int V,
                                    hipStream_t st);

// skinny_gemm.hip
void lumen_set_gemv_form(int form);
hipError_t lumen_skinny_swiglu_gemm(int dtype, const void* gu, const void* W, void* y, int M, int N,
                                    int K, long long ldgu, long long ldy, hipStream_t st);
hipError_t lumen_skinny_gemm(int dtype, const void* x, const void* W, void* y, int M, int N, int K,
                             long long ldx, long long ldy, hipStream_t st);

// swiglu.hip
hipError_t lumen_swiglu(int dtype, int bwd, const void* gu, const void* dact, void* out, int rows,
                        int F, int c0, int c1, hipStream_t st);

// transpose.hip
hipError_t lumen_transpose(int dtype, const void* in, void* out, int R, int C, long long ldi,
                           long long ldo, hipStream_t st);

// w4a16_gemm.hip
hipError_t lumen_w4a16_gemv(int dtype, const void* x, const void* W, const void* scale, void* y,
                            int M, int N, int K, long long ldx, long long ldy, int cfg,
                            hipStream_t st);
hipError_t lumen_w4a16_decode_gemm(int dtype, const void* x, const void* W, const void* scale,
                                   void* y, float* ws, int* cnt, int M, int N, int K, long long ldx,
                                   long long ldy, int BM, int BN, int S, hipStream_t st);

// w4a8_gemm.hip
hipError_t lumen_w4a8_decode_gemm(int dtype, const void* xq, const float* sx, const void* W,
                                  const void* scale, void* y, float* ws, int* cnt, int M, int N,
                                  int K, long long ldx, long long ldy, int BM, int BN, int S,
                                  hipStream_t st);
hipError_t lumen_w4_dequant(int dtype, const void* q, const void* scale, void* out, long long N,
                            long long K, hipStream_t st);

// w8_gemm.hip
hipError_t lumen_w8_gemv(int dtype, const void* x, const void* W, const float* scale, void* y,
                         int M, int N, int K, long long ldx, long long ldy, hipStream_t st);
hipError_t lumen_w8_decode_gemm(int dtype, const void* x, const void* W, const float* scale,
                                void* y, float* ws, int* cnt, int M, int N, int K, long long ldx,
                                long long ldy, int BM, int BN, int S, hipStream_t st);
hipError_t lumen_w8_dequant(int dtype, const void* q, const float* scale, void* out, long long N,
                            long long K, hipStream_t st);

// w8a8_gemm.hip
hipError_t lumen_act_quant_fp8(int dtype, const void* x, void* xq, float* sx, int M, int K,
                               long long ldx, hipStream_t st);
hipError_t lumen_w8a8_gemv(int dtype, const void* xq, const float* sx, const void* W,
                           const float* scale, void* y, int M, int N, int K, long long ldx,
                           long long ldy, hipStream_t st);
hipError_t lumen_w8a8_decode_gemm(int dtype, const void* xq, const float* sx, const void* W,
                                  const float* scale, void* y, float* ws, int* cnt, int M, int N,
                                  int K, long long ldx, long long ldy, int BM, int BN, int S,
                                  int form, hipStream_t st);
hipError_t lumen_w8a8_gemm(int dtype, const void* xq, const float* sx, const void* W,
                           const float* scale, void* y, int M, int N, int K, long long ldx,
                           long long ldy, hipStream_t st);

}  // extern "C"
