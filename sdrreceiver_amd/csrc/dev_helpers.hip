// dev_helpers.hip -- what every stage's kernels are written in: the address-space loads and stores, the packed complex
// arithmetic (v2f), the FIR multiply-accumulate statements, static_for, the buffer-resource stores and the lane helpers.
// No reference function of its own (cmul is libstdc++'s complex<float> operator* as vfo.cpp:241 and oscillator.cpp:22 use it).
// Relies on sdrx_dev.h only; every other file of kernels.hip relies on this one.

// ---- address spaces, vector types, global loads and stores ------------------------------------------------------------------
// Pointers that come out of a descriptor in memory are generic ("flat") to the compiler.  They
// all point into HBM: these helpers say so, so that accesses become global_load/global_store
// (or s_load for wave-uniform read-only data) instead of flat_* instructions.
#define SDRX_AS1 __attribute__((address_space(1)))
// Descriptors, work lists and filter taps are written at sdrx_finalize and never by a kernel that reads them
// (k_vfo_retune patches NCO fields and gains between frames, in a launch of its own): reading them through the
// CONSTANT address space tells the compiler so (no store of the kernel can alias them), and a wave-uniform address then becomes a scalar load into SGPRs whatever else the
// kernel does.  (Without it the 62 Hilbert taps of the demodulation turn into 62 VGPRs -- and spill --
// as soon as the same kernel also contains the mix/decimate code: k_frame.)
#define SDRX_AS4 __attribute__((address_space(4)))
template <typename T>
__device__ __forceinline__ T ldc(const T *p)
{
    return *(const SDRX_AS4 T *)p;
}
using v2f = float __attribute__((ext_vector_type(2)));
using v4f = float __attribute__((ext_vector_type(4)));
using v4s = short __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
__device__ __forceinline__ float gld(const float *p) { return *(const SDRX_AS1 float *)p; }
__device__ __forceinline__ float2 gld2(const float2 *p)
{
    const v2f v = *(const SDRX_AS1 v2f *)p;
    return make_float2(v.x, v.y);
}
__device__ __forceinline__ float4 gld4(const float4 *p)
{
    const v4f v = *(const SDRX_AS1 v4f *)p;
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void gst2(float2 *p, float2 a)
{
    v2f v = {a.x, a.y};
    *(SDRX_AS1 v2f *)p = v;
}
__device__ __forceinline__ void gst4(float4 *p, float4 a)
{
    v4f v = {a.x, a.y, a.z, a.w};
    *(SDRX_AS1 v4f *)p = v;
}

// ---- packed complex arithmetic ------------------------------------------------------------------
// Measured on MI355X (tools/valu_probe.hip): a plain fp32 VALU instruction issues every ~4.1 cycles
// per wave, a packed v_pk_{mul,add,fma}_f32 every ~4.4 -- so complex (re, im) pairs are kept as
// native 2-vectors and every operation is ONE packed instruction on both components.  Each packed
// lane is an ordinary IEEE fp32 operation, so EXACT results are unchanged.
__device__ __forceinline__ v2f xx(v2f a) { return __builtin_shufflevector(a, a, 0, 0); }
__device__ __forceinline__ v2f yy(v2f a) { return __builtin_shufflevector(a, a, 1, 1); }
__device__ __forceinline__ v2f yx(v2f a) { return __builtin_shufflevector(a, a, 1, 0); }
__device__ __forceinline__ v2f lo2(v4f a) { return __builtin_shufflevector(a, a, 0, 1); }
__device__ __forceinline__ v2f hi2(v4f a) { return __builtin_shufflevector(a, a, 2, 3); }
__device__ __forceinline__ v4f cat2(v2f a, v2f b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3); }
// (a.x b.x - a.y b.y, a.x b.y + a.y b.x) with every product and the final sum/difference rounded
// separately, like libstdc++'s complex<float> operator* (vfo.cpp:241, oscillator.cpp:22): the
// combine is fma(t2, (-1,+1), t1) -- multiplying by +-1 is exact, so it is one rounding, i.e. a
// subtraction in the low lane and an addition in the high lane.
__device__ __forceinline__ v2f cmul(v2f a, v2f b)
{
    const v2f t1 = xx(a) * b;
    const v2f t2 = yy(a) * yx(b);
    const v2f pm = {-1.0f, 1.0f};
    return __builtin_elementwise_fma(t2, pm, t1);
}
// One window sample w of a FIR feeding up to three accumulator chains: a_r += (h_r, h_r) * w with h_r = the low (H_r = 0) or
// high (H_r = 1) half of a PAIR of taps -- op_sel / op_sel_hi pick that half for both lanes of the packed instruction.
// (Written as `v2f{h, h} * w` the compiler materialises every pair (h, h) with two v_mov and the registers to hold them.)
// EXACT: product and sum rounded separately, the products first and the sums behind them so that no instruction waits for the
// one before it; all of it in ONE asm statement: a scheduler cannot pull the products of later samples up front (they do
// not depend on the accumulators: it did, and spilled them), and the hazard recogniser, which puts a wait state behind every
// asm statement whose result the next instruction reads, sees one statement per sample instead of one per product.
// Each lane of each instruction is an ordinary IEEE fp32 operation.
template <bool EXACT, int H0>
__device__ __forceinline__ void fir_mac1(v2f &a0, v2f h0, v2f w)
{
    v2f t0;
    if (EXACT)
        // (gfx950 wants one wait state between a packed fp32 instruction and a reader of its result -- the compiler puts an
        // s_nop there in its own code; inside an asm statement nobody does.  With two or three chains the other products are
        // that wait state.)
        asm("v_pk_mul_f32 %1, %2, %3 op_sel:[%4,0] op_sel_hi:[%4,1]\n\ts_nop 0\n\tv_pk_add_f32 %0, %0, %1" : "+v"(a0), "=&v"(t0) : "v"(h0), "v"(w), "n"(H0));
    else
        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[%3,0,0] op_sel_hi:[%3,1,1]" : "+v"(a0) : "v"(h0), "v"(w), "n"(H0));
}
template <bool EXACT, int H0, int H1>
__device__ __forceinline__ void fir_mac2(v2f &a0, v2f &a1, v2f h0, v2f h1, v2f w)
{
    v2f t0, t1;
    if (EXACT)
        asm("v_pk_mul_f32 %2, %4, %6 op_sel:[%7,0] op_sel_hi:[%7,1]\n\tv_pk_mul_f32 %3, %5, %6 op_sel:[%8,0] op_sel_hi:[%8,1]\n\t"
            "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3"
            : "+v"(a0), "+v"(a1), "=&v"(t0), "=&v"(t1)
            : "v"(h0), "v"(h1), "v"(w), "n"(H0), "n"(H1));
    else
        asm("v_pk_fma_f32 %0, %2, %4, %0 op_sel:[%5,0,0] op_sel_hi:[%5,1,1]\n\tv_pk_fma_f32 %1, %3, %4, %1 op_sel:[%6,0,0] op_sel_hi:[%6,1,1]"
            : "+v"(a0), "+v"(a1)
            : "v"(h0), "v"(h1), "v"(w), "n"(H0), "n"(H1));
}
template <bool EXACT, int H0, int H1, int H2>
__device__ __forceinline__ void fir_mac3(v2f &a0, v2f &a1, v2f &a2, v2f h0, v2f h1, v2f h2, v2f w)
{
    v2f t0, t1, t2;
    if (EXACT)
        asm("v_pk_mul_f32 %3, %6, %9 op_sel:[%10,0] op_sel_hi:[%10,1]\n\tv_pk_mul_f32 %4, %7, %9 op_sel:[%11,0] op_sel_hi:[%11,1]\n\t"
            "v_pk_mul_f32 %5, %8, %9 op_sel:[%12,0] op_sel_hi:[%12,1]\n\t"
            "v_pk_add_f32 %0, %0, %3\n\tv_pk_add_f32 %1, %1, %4\n\tv_pk_add_f32 %2, %2, %5"
            : "+v"(a0), "+v"(a1), "+v"(a2), "=&v"(t0), "=&v"(t1), "=&v"(t2)
            : "v"(h0), "v"(h1), "v"(h2), "v"(w), "n"(H0), "n"(H1), "n"(H2));
    else
        asm("v_pk_fma_f32 %0, %3, %6, %0 op_sel:[%7,0,0] op_sel_hi:[%7,1,1]\n\tv_pk_fma_f32 %1, %4, %6, %1 op_sel:[%8,0,0] op_sel_hi:[%8,1,1]\n\t"
            "v_pk_fma_f32 %2, %5, %6, %2 op_sel:[%9,0,0] op_sel_hi:[%9,1,1]"
            : "+v"(a0), "+v"(a1), "+v"(a2)
            : "v"(h0), "v"(h1), "v"(h2), "v"(w), "n"(H0), "n"(H1), "n"(H2));
}

// ---- static_for-------------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, 0>{}), ..., f(integral_constant<int, N - 1>{}): a loop whose index is a constant EXPRESSION
// inside the body (the op_sel digits above are template arguments)
template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f)
{
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// ---- vector loads and stores; stores through a buffer resource --------------------------------------------------------------
__device__ __forceinline__ v2f gldv2(const float2 *p) { return *(const SDRX_AS1 v2f *)p; }
__device__ __forceinline__ v4f gldv4(const float4 *p) { return *(const SDRX_AS1 v4f *)p; }
typedef unsigned v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4u gldv4u(const v4u *p) { return *(const SDRX_AS1 v4u *)p; }
// Four dongle bytes of one word -> two complex samples: floats[b] = b - 127 (jonti/sdr.cpp:43-49,122-129; sdrj.cpp:155-160).
// The one place the table is spelled out on the device, for ingest.hip (sample_pair) and mix.hip (load_run_raw).
__device__ __forceinline__ float4 cu8_pair(unsigned w)
{
    return make_float4((float)((int)(w & 255u) - 127), (float)((int)((w >> 8) & 255u) - 127), (float)((int)((w >> 16) & 255u) - 127),
                       (float)((int)(w >> 24) - 127));
}
__device__ __forceinline__ void gstv2(float2 *p, v2f v) { *(SDRX_AS1 v2f *)p = v; }
__device__ __forceinline__ void gstv4(float4 *p, v4f v) { *(SDRX_AS1 v4f *)p = v; }
// Stores that are ALWAYS issued, lanes that have nothing to store included: a buffer store whose offset lies beyond the
// resource's num_records is dropped by the hardware, so "this lane does not store" is an offset, not a branch -- and a
// store the compiler can see on every path is one it can COUNT: the s_waitcnt for loads issued in front of it then leaves
// it outstanding (vmcnt(n) with the stores among the n) instead of waiting for its acknowledgement.
typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
constexpr unsigned kNoStore = 0x7fffffffu; // a byte offset beyond every stream: the lane's store is dropped
__device__ __forceinline__ __amdgpu_buffer_rsrc_t stream_rsrc(float2 *base)
{
    return __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7ffffffe, 0x00020000); // raw buffer, no stride / swizzle, 32-bit data format
}
__device__ __forceinline__ void bst2(__amdgpu_buffer_rsrc_t r, unsigned byte_off, v2f v)
{
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i, v), r, (int)byte_off, 0, 0);
}
__device__ __forceinline__ void bst4(__amdgpu_buffer_rsrc_t r, unsigned byte_off, v4f v)
{
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, v), r, (int)byte_off, 0, 0);
}

// Loads through a resource that ends where the data does: a dword whose offset lies at or beyond num_records reads 0.0f, so
// "is this sample inside the frame" is the descriptor's business, not a compare and a branch per load.  The lane's whole
// byte offset goes into the VGPR operand -- the range check looks at that operand (and the instruction's 12-bit offset) only,
// never at a scalar offset.
constexpr unsigned kNoLoad = kNoStore; // a byte offset beyond every stream: the lane reads zeros
__device__ __forceinline__ __amdgpu_buffer_rsrc_t window_rsrc(const float2 *base, int samples)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float2 *>(base), 0, 8 * samples, 0x00020000);
}
__device__ __forceinline__ v4f bld4(__amdgpu_buffer_rsrc_t r, unsigned byte_off)
{
    return __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 0));
}

// ---- lane helpers -----------------------------------------------------------------------------------------------------------
// Whole-wave DPP shift by one lane (GFX9 `wave_shr:1`): lane l receives src of lane l-1,
// lane 0 keeps `old`.  Lane semantics verified on gfx950 by tools/dpp_probe.hip.
__device__ __forceinline__ float shr1(float old, float src)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src),
                                                                 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ v2f shr1(v2f old, v2f src)
{
    v2f r = {shr1(old.x, src.x), shr1(old.y, src.y)};
    return r;
}

// k_mix_decimate is ONE wave per workgroup and every LDS byte it touches is private to that wave.
// A wave's LDS instructions execute in program order, so a write by one lane is visible to a later
// read by another lane without any wait; all that is needed between phases is that the COMPILER
// keeps the order.  __syncthreads() would do that too, but it also emits s_waitcnt vmcnt(0): every
// phase boundary would drain the global loads and stores in flight (ten times per chunk).
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
