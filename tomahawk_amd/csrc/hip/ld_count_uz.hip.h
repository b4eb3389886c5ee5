// The (U, Z) form of the three-product contraction (included by ld_count.hip.h, whose A-side macros and register layout it shares).
//
// The r2 screen reads a pair through HH and S = QH + HQ + 2 QQ (contract3_chunk).  H and Q of a variant are disjoint and no genotype
// is missing, so per sample, and therefore over any K range,
//     HH = hA + hB - U,    U = popc(H_A | H_B)                              (inclusion - exclusion)
//     S  = qA + qB - Z,    Z = popc((Q_A ^ Q_B) & ~(H_A | H_B))             (the samples that are opposite homozygotes)
// with hA, qA, hB, qB the rows' popcounts over the same range (ld_two_screen.h: uz_to_hh_s turns the one into the other, in integers).
// U's operand is the third input of Z's: a word of a pair is v_or_b32, v_bcnt, v_bitop3_b32 (truth table 0x14 = (a ^ b) & ~c), v_bcnt -
// two popcounts where the product form has three, 12 SIMD cycles for 18.  Zero padding adds nothing to either count.
//
// Registers: the A sets P and R of contract3_chunk (whole slots by ds_read_b128: H tuples on registers = 0, Q tuples on registers = 2
// mod 4), so word k of a slot has hA in bank k and qA in bank k + 2.  The v_bitop3 reads qA, qB and the v_or's result, which must lie in
// three banks; the v_or itself does not care.  The B pairs therefore need no word swap any more: they are read by plain ds_read_b64 -
// half the LDS cycles of the product form's ds_read2_b32, and LDS bandwidth is what this loop has least of - with the Q pair of a
// slot's lower half on a register = 0 and of its upper half on a register = 2 (mod 4): qB of word k lies in bank k + 2 + 2 = k, the
// temporary of words 0 and 2 in bank 1 (v125), that of words 1 and 3 in bank 0 (v124).  The v_bitop3 writes its third source in place.
#pragma once

// one word of one variant pair: U += popc(hA | hB), Z += popc((qA ^ qB) & ~(hA | hB)); HA / QA: first register of the A variant's H / Q tuple, K: the word of the slot
// ((op, s_nop 0, v_bcnt) as in and_bcnt8v; csrc/tools/uz_probe.hip: 94.4 - 96.4 % of the 12-cycle ceiling in a register-only stream, 72 % without the s_nop, 81 % with one of
// the two; in this kernel at 1024 tiles of 977 chunks: 12.59 ms with both, 13.16 with the second only, 13.43 with a third in front of the v_bitop3, 14.14 with none)
#define TWK_UZ_PR(T, HA, QA, K, HB, QB, U, Z) "v_or_b32 v" #T ", v[" #HA "+" #K "], v" #HB "\n\ts_nop 0\n\tv_bcnt_u32_b32 %[" #U "], v" #T ", %[" #U "]\n\t" \
	"v_bitop3_b32 v" #T ", v[" #QA "+" #K "], v" #QB ", v" #T " bitop3:0x14\n\ts_nop 0\n\tv_bcnt_u32_b32 %[" #Z "], v" #T ", %[" #Z "]\n\t"
// one B variant V against the lane's four A variants (H tuples from register H on, Q tuples from Q on, four registers a variant), words KX and KY of the
// slot in turn, so that consecutive pairs use the two temporaries in turn (the probe: 96.4 against 94.4 % of the ceiling)
#define TWK_UZ_G8(H, Q, KX, KY, HBX, QBX, HBY, QBY, V) \
	TWK_UZ_PR(125, H, Q, KX, HBX, QBX, h0##V, s0##V) TWK_UZ_PR(124, H+4, Q+4, KY, HBY, QBY, h1##V, s1##V) TWK_UZ_PR(125, H+8, Q+8, KX, HBX, QBX, h2##V, s2##V) TWK_UZ_PR(124, H+12, Q+12, KY, HBY, QBY, h3##V, s3##V) \
	TWK_UZ_PR(124, H, Q, KY, HBY, QBY, h0##V, s0##V) TWK_UZ_PR(125, H+4, Q+4, KX, HBX, QBX, h1##V, s1##V) TWK_UZ_PR(124, H+8, Q+8, KY, HBY, QBY, h2##V, s2##V) TWK_UZ_PR(125, H+12, Q+12, KX, HBX, QBX, h3##V, s3##V)
// B set X (a slot's lower half): qB0 v108 v109, hB0 v110 v111, qB1 v112 v113, hB1 v114 v115; Y (upper half): hB0 v116 v117, qB0 v118 v119, hB1 v120 v121, qB1 v122 v123
#define TWK_UZ_HALF0(H, Q) TWK_UZ_G8(H, Q, 0, 1, 110, 108, 111, 109, 0) TWK_UZ_G8(H, Q, 0, 1, 114, 112, 115, 113, 1)
#define TWK_UZ_HALF1(H, Q) TWK_UZ_G8(H, Q, 2, 3, 116, 118, 117, 119, 0) TWK_UZ_G8(H, Q, 2, 3, 120, 122, 121, 123, 1)
#define TWK_UZ_HALF0_P TWK_UZ_HALF0(36, 54)
#define TWK_UZ_HALF1_P TWK_UZ_HALF1(36, 54)
#define TWK_UZ_HALF0_R TWK_UZ_HALF0(72, 90)
#define TWK_UZ_HALF1_R TWK_UZ_HALF1(72, 90)
#define TWK_UZ_RD_B(LO, HI, OFF) "ds_read_b64 v[" #LO ":" #HI "], %[aB] offset:" #OFF "\n\t"
#define TWK_UZ_READ_BX TWK_UZ_RD_B(110, 111, 0) TWK_UZ_RD_B(108, 109, 128) TWK_UZ_RD_B(114, 115, 2048) TWK_UZ_RD_B(112, 113, 2176)
#define TWK_UZ_READ_BY TWK_UZ_RD_B(116, 117, 8) TWK_UZ_RD_B(118, 119, 136) TWK_UZ_RD_B(120, 121, 2056) TWK_UZ_RD_B(122, 123, 2184)
#define TWK_UZ_CLOBBER_T "v124", "v125"
#define TWK_UZ_SLOT_ADDR(Q16) "v_xor_b32 %[aA], " #Q16 ", %[bA]\n\tv_xor_b32 %[aB], " #Q16 ", %[bB]\n\t"
// (the order of contract3_chunk's TWK_SLOT: the upper half's B pairs in front of the lower half's pairs of words, all of the next slot in front of the upper half's)
#define TWK_UZ_SLOT(CUR, NXT, NEXT_Q16) TWK_UZ_READ_BY "s_waitcnt lgkmcnt(4)\n\t" TWK_UZ_HALF0_##CUR TWK_UZ_SLOT_ADDR(NEXT_Q16) TWK_READ_##NXT TWK_UZ_READ_BX "s_waitcnt lgkmcnt(12)\n\t" TWK_UZ_HALF1_##CUR
#define TWK_UZ_ACCS(acc) [h00] "+v"(acc[0][0]), [h01] "+v"(acc[0][2]), [h10] "+v"(acc[2][0]), [h11] "+v"(acc[2][2]), [h20] "+v"(acc[4][0]), [h21] "+v"(acc[4][2]), \
	[h30] "+v"(acc[6][0]), [h31] "+v"(acc[6][2]), [s00] "+v"(acc[1][1]), [s01] "+v"(acc[1][3]), [s10] "+v"(acc[3][1]), [s11] "+v"(acc[3][3]), \
	[s20] "+v"(acc[5][1]), [s21] "+v"(acc[5][3]), [s30] "+v"(acc[7][1]), [s31] "+v"(acc[7][3])

namespace twk {

// A whole chunk: U where contract3_chunk leaves HH (acc[2 s][2 v]), Z where it leaves S (acc[2 s + 1][2 v + 1]).
__device__ __forceinline__ void contract_uz_chunk(uint32_t (&acc)[8][4], uint32_t bA, uint32_t bB) {
	static_assert(KC * 4 == 128 && lane_row_offset<true, 1>() == 128 && lane_row_offset<true, 2>() == 2048 && lane_row_offset<true, 3>() == 2176, "the offsets in TWK_UZ_READ_BX / _BY");
	uint32_t aA, aB;
	asm volatile(TWK_UZ_SLOT_ADDR(0) TWK_READ_P TWK_UZ_READ_BX
	             TWK_UZ_SLOT(P, R, 16) TWK_UZ_SLOT(R, P, 32) TWK_UZ_SLOT(P, R, 48) TWK_UZ_SLOT(R, P, 64) TWK_UZ_SLOT(P, R, 80) TWK_UZ_SLOT(R, P, 96) TWK_UZ_SLOT(P, R, 112)
	             TWK_UZ_READ_BY "s_waitcnt lgkmcnt(4)\n\t" TWK_UZ_HALF0_R "s_waitcnt lgkmcnt(0)\n\t" TWK_UZ_HALF1_R
	             : TWK_UZ_ACCS(acc), [aA] "=&v"(aA), [aB] "=&v"(aB)
	             : [bA] "v"(bA), [bB] "v"(bB)
	             : "memory", TWK_CLOBBER_P, TWK_CLOBBER_R, TWK_CLOBBER_B, TWK_UZ_CLOBBER_T);
}

// One slot the plain way (reads, wait, pairs of words): the last chunk of rows that end inside it, as contract3_slot.
__device__ __forceinline__ void contract_uz_slot(uint32_t (&acc)[8][4], uint32_t aA, uint32_t aB) {
	asm volatile(TWK_READ_P TWK_UZ_READ_BX TWK_UZ_READ_BY "s_waitcnt lgkmcnt(0)\n\t" TWK_UZ_HALF0_P TWK_UZ_HALF1_P
	             : TWK_UZ_ACCS(acc)
	             : [aA] "v"(aA), [aB] "v"(aB)
	             : "memory", TWK_CLOBBER_P, TWK_CLOBBER_B, TWK_UZ_CLOBBER_T);
}

}      // namespace twk
