// Dev tool: what does the (U, Z) form's word of a pair (ld_count_uz.hip.h) reach in a register-only stream?
//   U += popc(hA | hB),  Z += popc((qA ^ qB) & ~(hA | hB))  -  v_or_b32, v_bcnt, v_bitop3_b32 (truth table 0x14), v_bcnt: 2 + 4 + 2 + 4 SIMD cycles
// (1) the truth table's convention, checked on random words against (a ^ b) & ~c;
// (2) the issue rate of the group under the s_nop placements, temporaries and banks of uz_probe_gen.py, 4 waves per SIMD (512-thread blocks,
//     two per CU, like the count kernel), as a fraction of the 12-cycle ceiling 256 CU x 4 SIMD x 64 / 12 x 2.4 GHz = 1.31e13 words of pairs a second.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "uz_probe_gen.h"
#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){fprintf(stderr,"HIP %s: %s\n",#x,hipGetErrorString(e)); exit(1);} }while(0)
#define CLOB "v32","v33","v34","v35","v36","v37","v38","v39","v40","v41","v42","v43","v44","v45","v46","v47","v48","v49","v50","v51","v52","v53","v54","v55","v56","v57","v58","v59","v60","v61","v62","v63","v64","v65","v66","v67","v68","v69","v70","v71"
#define R8(X) X X X X X X X X
template<int MODE> __global__ __launch_bounds__(512, 2) void k(uint32_t* out, int iters){
  for(int it=0; it<iters; ++it){
    if(MODE==0) asm volatile(R8(UZ_NOP_BOTH) ::: CLOB);
    else if(MODE==1) asm volatile(R8(UZ_NOP_BOTH_ALT) ::: CLOB);
    else if(MODE==2) asm volatile(R8(UZ_NOP_NONE) ::: CLOB);
    else if(MODE==3) asm volatile(R8(UZ_NOP_OR) ::: CLOB);
    else if(MODE==4) asm volatile(R8(UZ_NOP_BITOP) ::: CLOB);
    else if(MODE==5) asm volatile(R8(UZ_NOP_ALL) ::: CLOB);
    else if(MODE==6) asm volatile(R8(UZ_BANK_CLASH) ::: CLOB);
    else if(MODE==7) asm volatile(R8(UZ_RESULT_APART) ::: CLOB);
    else if(MODE==8) asm volatile(R8(UZ_PAIRED) ::: CLOB);
    else asm volatile(R8(UZ_PAIRED_NOP) ::: CLOB);
  }
  uint32_t s; asm volatile("v_add_u32 %0, v64, v68" : "=v"(s)); out[blockIdx.x*blockDim.x+threadIdx.x]=s;
}
template<int MODE> void run(const char* name){
  int blocks=256*2; uint32_t* d; CK(hipMalloc(&d,(size_t)blocks*512*4));
  int iters=20000; hipEvent_t e0,e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  hipLaunchKernelGGL((k<MODE>),dim3(blocks),dim3(512),0,0,d,2000); CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0)); hipLaunchKernelGGL((k<MODE>),dim3(blocks),dim3(512),0,0,d,iters); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
  float ms; CK(hipEventElapsedTime(&ms,e0,e1));
  const double words=(double)blocks*512*iters*8*8;      // (8 streams of 8 words of pairs an iteration)
  printf("%-66s %.3f ms  words of pairs/s %.3e (%.1f %% of the 12-cycle ceiling 1.31e13)\n",name,ms,words/ms*1e3,words/ms*1e3/1.3107e13*100); fflush(stdout);
  CK(hipFree(d));
}
__global__ void k_check(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* o, int n){
  const int i=blockIdx.x*blockDim.x+threadIdx.x; if(i>=n) return;
  uint32_t r; asm volatile("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x14" : "=v"(r) : "v"(a[i]), "v"(b[i]), "v"(c[i]));
  o[i]=r;
}
int main(){
  const int n=1<<20; std::vector<uint32_t> a(n),b(n),c(n),o(n); std::mt19937 rng(3); for(int i=0;i<n;++i){a[i]=rng();b[i]=rng();c[i]=rng();}
  uint32_t *da,*db,*dc,*dout; CK(hipMalloc(&da,n*4)); CK(hipMalloc(&db,n*4)); CK(hipMalloc(&dc,n*4)); CK(hipMalloc(&dout,n*4));
  CK(hipMemcpy(da,a.data(),n*4,hipMemcpyHostToDevice)); CK(hipMemcpy(db,b.data(),n*4,hipMemcpyHostToDevice)); CK(hipMemcpy(dc,c.data(),n*4,hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_check,dim3(n/256),dim3(256),0,0,da,db,dc,dout,n); CK(hipMemcpy(o.data(),dout,n*4,hipMemcpyDeviceToHost));
  int bad=0; for(int i=0;i<n;++i) if(o[i]!=((a[i]^b[i])&~c[i])) ++bad;
  printf("v_bitop3_b32 bitop3:0x14 == (a ^ b) & ~c: %d mismatches of %d words\n",bad,n);
  run<0>("(or, s_nop, bcnt, bitop3, s_nop, bcnt), the sources in three banks");
  run<1>("... two temporaries in turn");
  run<2>("... no s_nop");
  run<3>("... s_nop behind the v_or only");
  run<4>("... s_nop behind the v_bitop3 only");
  run<5>("... a third s_nop between the first v_bcnt and the v_bitop3");
  run<6>("... the temporary in qA's bank");
  run<7>("... the v_bitop3 writes another register than its third source");
  run<8>("two words interleaved (or or bcnt bcnt bitop3 bitop3 bcnt bcnt)");
  run<9>("... an s_nop between the four pairs");
  return bad!=0;
}
