// The fused Monte-Carlo inference kernel (NTF_INFER_MC=1) in a translation unit of its own: the code object of ntf_fused.hip - every kernel of the default paths -
// stays what it was before this kernel existed.
#include "ntf_fused_common.h"

namespace ntf {

// ------------------------------------------------------------------------------------------------
// k_out_probs_mc (NTF_INFER_MC=1): the Flipout inference form of k_out_fwd_b6 (<true, false, false, false, PROBS>) with the Monte-Carlo passes INSIDE the kernel.
// k_out_fwd_b6 reads and rewrites every running sum of the transposed [experts x batch] buffer once per pass (pold: 0.93 GB each way at config 2, B = 1000); here a
// column group walks its 32-expert tiles in groups of MC_G, the pass loop outside the tile loop, and a group's running sums - 16 registers a tile, in the registers
// k_out_fwd_b6 keeps for Y1 / Y2 - are stored once, behind the launch's last pass.  At the head of each pass of a group the wave reloads and splits its h operand
// from that pass's zero-padded image (64 KB a workgroup from L2; MC_G tiles of matrix work amortise it) and hashes that pass's s_in words.  Per (tile, pass): the
// planes of mu, of that pass's sigma * eps and both bias tiles are staged as in k_out_fwd_b6; MFMA order, u_z, bias add, s_out hash and the unclamped logit are the
// same statements, and acc = fmaf(pr, pscale, acc) runs in pass order from pold (pacc: an earlier launch's passes) or 0 - the probabilities are bit-identical to the
// per-pass path's.  The launch covers the 32-expert tiles [t_lo, t_hi) of the layer: mu_pl, the passes' planes and bp slots hold that range only (tile t_lo first),
// mu_b, dzT, M and the s_out hash keep the layer's numbering.  Entropy terms of every pass go into the one LossAcc; the slot (row, cg_off + cg) of ncg_tot is
// added to when pacc is set.
// Occupancy: ONE workgroup per CU (the training step's column groups, geom().NCG), not the two of k_out_fwd_b6's forward-only launches (eval_ncg).  The register
// budget decides: beside the h planes (64), the zT accumulators (32) and the fragments in flight, hipcc places MC_G = 4 tiles of sums in 365 registers without a
// spill; held to the 256 of two workgroups per CU it spills 101 of them to scratch at MC_G = 4 and 6 at MC_G = 2 (k_out_fwd_b6's PROBS form already takes 199 of
// the 256: it keeps the 64 registers of h * s_in live, which this kernel rebuilds per use).  The two-workgroup form has not been timed; this one measured slower than
// the per-pass path at config 2 (profiles/infer_mc_bench.md: one wave per SIMD issues its MFMAs and its epilogue in order), hence opt-in.
// ------------------------------------------------------------------------------------------------
struct McPassArgs { const float* h; const uint16_t* wp_pl; const float* bp; uint32_t so_k0, so_k1, si_k0, si_k1; };
struct McBase { OutFwdArgs a; const uint16_t* mu_pl; float h_scale, u_z; };      // (k_out_fwd_b6's OutFwd6Args without what only training reads)
struct OutProbsMcArgs { McBase b; int npass; McPassArgs ps[kMcMaxGroup]; };

__global__ __launch_bounds__(256, 1) void k_out_probs_mc(OutProbsMcArgs pp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const OutFwdArgs& p = pp.b.a;
    constexpr int H = 128, NJT = 4, NKS = H / 16, G = MC_G;
    constexpr int PLANE = BN6 * H * 2, TM = 2 * PLANE, STAGE = 2 * TM + 512;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, il = lane & 31, half = lane >> 5;
    if (range_guard_skip(p.rflag, p.rmode, false)) return;

    int bid = blockIdx.x;
    const int nblk = gridDim.x;
    if ((nblk & 7) == 0) bid = (bid & 7) * (nblk >> 3) + (bid >> 3);
    const int cg = bid / p.NRB, rb = bid % p.NRB;
    const int nt = p.t_hi - p.t_lo;
    const int t_beg = p.t_lo + (int)((int64_t)cg * nt / p.NCG), t_end = p.t_lo + (int)((int64_t)(cg + 1) * nt / p.NCG);
    const int i0 = rb * BM + wave * 32;
    const int i = i0 + il;
    const bool row_ok = i < p.B;
    const float rmask = row_ok ? 1.f : 0.f;
    const int np = pp.npass;
    const int fil = ((il & 3) << 2) | ((il >> 2) & 3);

    const uint32_t smem_base = lds_addr(smem);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto stage_tile = [&](int t, int ps, int buf) {      // tile t of pass ps -> LDS stage buf
        const McPassArgs& q = pp.ps[ps];
        const uint32_t sb = smem_base + buf * STAGE;
        constexpr int PER_WAVE = TM / 1024 / 4;
#pragma unroll
        for (int n = 0; n < PER_WAVE; ++n) {
            const int inst = wave_u * PER_WAVE + n;
            const int pos = inst * 1024 + lane * 16;
            const int row = (pos >> 8) & 31, chp = (pos >> 4) & 15;
            const int ch = chp ^ (((row & 3) << 2) | ((row >> 2) & 3));
            const size_t src = (size_t)(t - p.t_lo) * TM + (pos & ~255) + 16 * ch;
            glds16(reinterpret_cast<const char*>(pp.b.mu_pl) + src, sb + inst * 1024);
            glds16(reinterpret_cast<const char*>(q.wp_pl) + src, sb + TM + inst * 1024);
        }
        const int c = min(t * BN6 + lane, min(p.M, p.t_hi * BN6) - 1);      // (a bias tile is 64 floats: never past the range the bp slot holds)
        if (wave_u == 0) glds4(p.mu_b + c, sb + 2 * TM);
        if (wave_u == 1) glds4(q.bp + (c - p.t_lo * BN6), sb + 2 * TM + 256);
    };
    LossAcc lacc;
    if (t_beg < t_end) stage_tile(t_beg, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int it = 0;      // (tile, pass) items done: the LDS stage of the current one is it & 1
    for (int tg = t_beg; tg < t_end; tg += G) {
        const int ng = min(G, t_end - tg);
        f32x16 acc[G];         // the running sums of the group's tiles
        for (int ps = 0; ps < np; ++ps) {
            const McPassArgs& q = pp.ps[ps];
            // B operand of zT for this pass: h[i][16s + 8*half + e] split into planes; its s_in sign words
            u32x4 hp[NKS][2];
            uint32_t sinw[NJT];
#pragma unroll
            for (int w = 0; w < NJT; ++w) sinw[w] = row_ok ? sign_word(q.si_k0, q.si_k1, (uint32_t)i, (uint32_t)w) : 0u;
#pragma unroll
            for (int s = 0; s < NKS; ++s) {
                const float4 v0 = *reinterpret_cast<const float4*>(q.h + (int64_t)i * H + 16 * s + 8 * half);   // zero-padded to Bpad rows
                const float4 v1 = *reinterpret_cast<const float4*>(q.h + (int64_t)i * H + 16 * s + 8 * half + 4);
                const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t pq[2];
                    split_pair_scaled(x[2 * k], x[2 * k + 1], pp.b.h_scale, pq);
                    hp[s][0][k] = pq[0]; hp[s][1][k] = pq[1];
                }
            }
            const bool first = ps == 0, last = ps == np - 1;
            static_for<0, G>([&](auto gc) {
                constexpr int g = decltype(gc)::value;
                if (g >= ng) return;      // (workgroup-uniform)
                const int t = tg + g;
                const int buf = it & 1; ++it;
                const uint32_t sw = (row_ok ? sign_word(q.so_k0, q.so_k1, (uint32_t)i, (uint32_t)t) : 0u) >> (4 * half);
                // the next item: the group's next tile, else the group's first tile of the next pass, else the next group's first tile of pass 0
                if (g + 1 < ng) stage_tile(t + 1, ps, buf ^ 1);
                else if (!last) stage_tile(tg, ps + 1, buf ^ 1);
                else if (tg + G < t_end) stage_tile(tg + G, 0, buf ^ 1);
                char* sb = smem + buf * STAGE;
                const int c0 = t * BN6;
                if (c0 + BN6 > p.M) {  // ragged last tile (workgroup-uniform): mask the experts past M through their bias
                    if (tid < BN6 && c0 + tid >= p.M) reinterpret_cast<float*>(sb + 2 * TM)[tid] = -1e30f;
                    __syncthreads();
                }
                f32x16 X1, X2;
#pragma unroll
                for (int r = 0; r < 16; ++r) { X1[r] = 0.f; X2[r] = 0.f; }
                constexpr int dz_row_bytes = 128;   // dzT tile layout, see dzt_index
                const __amdgpu_buffer_rsrc_t dz_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.dzT + dzt_tile_base(c0, p.Bpad), 0, ((p.Bpad >> 5) * 8192 - ((c0 & 255) << 5)) * 4, 0x00020000);
                const int dz_voff = ((i >> 5) * 8192 + 4 * half * 32 + (i & 31)) * 4;
                if (first) {      // the sums an earlier launch's passes left (pacc), fetched under the zT products
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc[g][r] = p.pacc ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(dz_rsrc, dz_voff, ((r & 3) + 8 * (r >> 2)) * dz_row_bytes, 0)) : 0.f;
                }
                // ---- zT = mu . hT + Wp . (h*s_in)T, as in k_out_fwd_b6
                {
                    constexpr int NHG = NKS * 2;
                    auto z_load = [&](int hg, u32x4 (&fr)[2]) {
                        const int s = hg / 2, mat = hg % 2;
                        const char* ap = sb + 256 * il + 16 * ((2 * s + half) ^ fil) + mat * TM;
#pragma unroll
                        for (int k = 0; k < 2; ++k) fr[k] = *reinterpret_cast<const u32x4*>(ap + k * PLANE);
                    };
                    u32x4 fr[2][2];
                    z_load(0, fr[0]);
#pragma unroll
                    for (int hg = 0; hg < NHG; ++hg) {
                        if (hg + 1 < NHG) z_load(hg + 1, fr[(hg + 1) & 1]);
                        asm volatile("" ::: "memory");
                        const int s = hg / 2, mat = hg % 2;
                        if (mat == 0) X1 = mfma3h(fr[hg & 1], hp[s], X1);
                        else {
                            u32x4 hs[2];
                            uint32_t w8 = sinw[s >> 1] >> (16 * (s & 1) + 8 * half);
                            asm volatile("" : "+v"(w8));      // signed operand made per use: hipcc would keep all 64 registers of h * s_in live across the group's tiles
                            u32x4 hm;
#pragma unroll
                            for (int k = 0; k < 4; ++k) hm[k] = ((w8 << (15 - 2 * k)) & 0x8000u) | ((w8 << (30 - 2 * k)) & 0x80000000u);
#pragma unroll
                            for (int k = 0; k < 2; ++k) hs[k] = hp[s][k] ^ hm;
                            X2 = mfma3h(fr[hg & 1], hs, X2);
                        }
                    }
                }
                // ---- epilogue: lane = batch row i, register r <-> expert c0 + rowmap(r, half)
                const float* bias_mu = reinterpret_cast<const float*>(sb + 2 * TM) + 4 * half;
                const float* bias_p = reinterpret_cast<const float*>(sb + 2 * TM + 256) + 4 * half;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int cr = (r & 3) + 8 * (r >> 2);
                    float z = fmaf(X1[r], pp.b.u_z, bias_mu[cr]);
                    z += __uint_as_float(__float_as_uint(fmaf(X2[r], pp.b.u_z, bias_p[cr])) ^ ((sw << (31 - cr)) & 0x80000000u));
                    const float l = z > 0.f ? z : z * kLeakySlope;
                    const float tt = 1.f + __builtin_amdgcn_exp2f(l * -1.4426950408889634f);
                    const float pr = __builtin_amdgcn_rcpf(tt) * rmask;       // experts past M: bias -1e30 -> tt = +inf -> 0
                    lacc.tile = fmaf(-pr * 0.6931471805599453f, __builtin_amdgcn_logf(pr + 1e-15f), lacc.tile);
                    acc[g][r] = fmaf(pr, p.pscale, acc[g][r]);
                    if (last) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[g][r]), dz_rsrc, dz_voff, cr * dz_row_bytes, 0);
                }
                lacc.end_tile();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            });
        }
    }

    // per-row entropy partial of this column group: the terms of every pass of this launch (+ an earlier launch's, pacc)
    float lsum = lacc.sum;
    lsum += __shfl_xor(lsum, 32, 64);
    if (half == 0) {
        float* slot = p.lossp + (int64_t)i * p.ncg_tot + p.cg_off + cg;
        *slot = p.pacc ? *slot + lsum : lsum;
    }
}

void launch_fused_probs_mc(hipStream_t st, const FusedProbsMc& f) {
    const Geom g = geom(f.B, f.M);
    OutProbsMcArgs a = {};
    OutFwdArgs& o = a.b.a;
    o.B = f.B; o.M = f.M; o.Bpad = g.Bpad; o.NRB = g.NRB; o.NCG = fused_mc_ncg(f.B, f.c_hi - f.c_lo); o.T = g.T; o.nCB = g.nCB;
    o.t_lo = f.c_lo / BN6; o.t_hi = (f.c_hi + BN6 - 1) / BN6; o.cg_off = f.cg_off; o.ncg_tot = f.ncg_tot;
    o.mu_b = f.mu_b; o.dzT = f.dzT; o.lossp = f.lossp; o.tnw = 1.f; o.inv_B = 1.f / (float)f.B;
    o.rflag = f.rflag; o.rmode = f.rflag ? 1 : 0; o.pscale = f.pscale; o.pacc = f.pacc; o.Hr = 128;
    a.b.mu_pl = f.mu_pl; a.b.h_scale = f.h_scale; a.b.u_z = 1.f / (f.w_scale * f.h_scale);
    a.npass = f.npass;
    for (int k = 0; k < f.npass; ++k) {
        const FusedMcPass& s = f.pass[k];
        a.ps[k] = McPassArgs{s.hz, s.wp_pl, s.bp, s.s_out.k0, s.s_out.k1, s.s_in.k0, s.s_in.k1};
    }
    launch_lds(k_out_probs_mc, dim3(g.NRB * o.NCG), dim3(256), fwd_b6_lds(true), st, a);
}

}  // namespace ntf
