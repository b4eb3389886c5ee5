// Stand-alone micro-benchmark + self-check of the count kernels (dev tool):
//   grid  k_count_tile_t   one block per 128 x 128 tile (2-D grid; the round-1 kernel)
//   list  k_count_list_t   persistent blocks over a tile list, data-parallel rounds + stream-K tail
// usage: count_microbench [rows=4096] [words=3136] [reps=3] [blocks=512]
//   ONLYMODE=2: only the list kernel in patch order on the rectangle (rocprofv3 counter passes)
//   NOSTORE=1: the list kernel without its epilogue (what the C stores cost: nothing measurable - 87.7 -> 88.3 % of the
//   ceiling at 5 chunks a tile; the self-check then fails by design)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <random>
#include "../hip/ld_count.hip.h"
#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){fprintf(stderr,"HIP %s @%d: %s\n",#x,__LINE__,hipGetErrorString(e)); exit(1);} }while(0)

// The table of the R x R rows (ld_count_table.h), on the device at dt.  patch: 8 x 8 patches as the engine walks them, else row by row (patches of one
// row of tiles); knobs: SHAREDIV / TAILROUNDS of the guided tail from the environment; fused: whole tiles only.
static twk::CountTable make_table(uint32_t R, uint32_t W, int diag, bool patch, uint32_t blocks, uint32_t min_chunks, uint32_t* dt, bool knobs = false, bool fused = false) {
	twk::CountSettings cs; cs.n_blocks = blocks; cs.min_chunks = min_chunks; cs.fused = fused;
	if (!patch) { cs.patch_rows = 1; cs.patch_cols = std::max(R / 128, 1u); }
	if (knobs && getenv("SHAREDIV")) cs.share_div = atoi(getenv("SHAREDIV"));
	if (knobs && getenv("TAILROUNDS")) cs.tail_rounds = atoi(getenv("TAILROUNDS"));
	const twk_hip_tile_desc t{0, R, 0, R, diag, 0, 0, 0};
	const twk::CountTable tb = twk::build_count_table(t, 1, diag != 0, nullptr, W / twk::KC, cs);
	std::vector<uint32_t> image(tb.words());
	tb.pack(image.data());
	CK(hipMemcpy(dt, image.data(), image.size() * 4, hipMemcpyHostToDevice));
	return tb;
}
int main(int argc,char**argv){
  uint32_t R = argc>1? atoi(argv[1]) : 4096;     // rows (multiple of 128)
  uint32_t W = argc>2? atoi(argv[2]) : 3136;     // words per row (multiple of 32)
  int reps = argc>3? atoi(argv[3]) : 3;
  uint32_t P = argc>4? atoi(argv[4]) : 512;      // persistent blocks
  size_t nw=(size_t)R*W;
  std::vector<uint32_t> h(nw); std::mt19937 rng(1); for(auto&x:h) x=rng();
  if(getenv("FUSED") && getenv("LIVE")) for(uint32_t r=0;r<R;++r) for(uint32_t k=atoi(getenv("LIVE"));k<W;++k) h[(size_t)r*W+k]=0;      // zero padding behind the live words
  if(getenv("FUSED")) for(uint32_t r=1;r<R;r+=2) for(uint32_t k=0;k<W;++k) h[(size_t)r*W+k] &= ~h[(size_t)(r-1)*W+k];   // rows 2v / 2v + 1 as a variant's H / Q planes: disjoint
  uint32_t *d,*C,*dt; CK(hipMalloc(&d,nw*4)); CK(hipMalloc(&C,(size_t)R*R*4)); CK(hipMalloc(&dt,(size_t)(R/128)*(R/128)*(4+(size_t)(W/twk::KC)*16)+65536));      // dt: room for every tile in units of one chunk
  const uint32_t min_chunks = getenv("MINCHUNKS")? atoi(getenv("MINCHUNKS")) : 8;
  CK(hipMemcpy(d,h.data(),nw*4,hipMemcpyHostToDevice)); CK(hipMemset(C,0xff,(size_t)R*R*4));
  dim3 grid(R/128,R/128), block(twk::COUNT_THREADS);
  hipEvent_t e0,e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  int bad_total=0;
  auto check=[&](const char* what,int diag){
    std::vector<uint32_t> hc((size_t)R*R); CK(hipMemcpy(hc.data(),C,(size_t)R*R*4,hipMemcpyDeviceToHost));
    int bad=0; std::mt19937 r2(7);
    for(int s=0;s<2000;++s){ uint32_t i=r2()%R,j=r2()%R; if(diag && j/128<i/128) continue; uint32_t ref=0; for(uint32_t k=0;k<W;++k) ref+=__builtin_popcount(h[(size_t)i*W+k]&h[(size_t)j*W+k]); if(ref!=hc[(size_t)i*R+j]){ if(bad<5) printf("MISMATCH %s (%u,%u) ref %u got %u\n",what,i,j,ref,hc[(size_t)i*R+j]); ++bad; } }
    printf("check %s: %d mismatches\n",what,bad); bad_total+=bad;
  };
  if(const char* gy=getenv("GRIDY")){   // probe: the 2-D grid kernel over gy tile rows only (e.g. 16 x 32 = 512 tiles = one round)
    const uint32_t ny=atoi(gy); dim3 g2(R/128,ny);
    hipLaunchKernelGGL((twk::k_count_tile_t<twk::COUNT_NW>),g2,block,0,0,d,W,0u,0u,0,C,R); CK(hipDeviceSynchronize());
    float best=1e30f;
    for(int i=0;i<reps;++i){ CK(hipEventRecord(e0)); hipLaunchKernelGGL((twk::k_count_tile_t<twk::COUNT_NW>),g2,block,0,0,d,W,0u,0u,0,C,R); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms,e0,e1)); if(ms<best)best=ms; }
    const double tiles=(double)(R/128)*ny, wordops=tiles*128*128*W;
    printf("grid %ux%u tiles=%.0f best %.3f ms  word-pairs/s %.3e (%.1f%% of the and+bcnt ceiling)\n",R/128,ny,tiles,best,wordops/best*1e3,wordops/best*1e3/2.6214e13*100);
    return 0;
  }
  uint32_t* tick; CK(hipMalloc(&tick,4));
  if(const char* bs=getenv("BASE_SWEEP")){   // probe: does the kernel's speed depend on where the rows lie?  The same rows at n different
    // offsets (multiples of STEP bytes, default 2 MiB - what separates one process's allocation from another's) inside one big
    // buffer; 3 warm launches, then the best of `reps`, per offset.
    const int n=atoi(bs); const size_t step=getenv("STEP")? strtoull(getenv("STEP"),nullptr,10) : (2ull<<20);
    uint8_t* big; CK(hipMalloc(&big,nw*4+(size_t)n*step));
    const twk::CountTable tb=make_table(R,W,0,true,P,min_chunks,dt);
    twk::CountWork w=twk::count_work(nullptr,W,0,0,dt,tb,C,R,tick,0,nullptr);
    std::vector<float> ms_all;
    for(int o=0;o<n;++o){
      uint32_t* base=reinterpret_cast<uint32_t*>(big+(size_t)o*step);
      CK(hipMemcpy(base,d,nw*4,hipMemcpyDeviceToDevice)); w.rows=base;
      float best=1e30f;
      for(int i=0;i<3+reps;++i){ CK(hipMemsetAsync(tick,0,4,0));
        CK(twk::enqueue_count(0,w,tb,P,128u,e0,twk::k_count_list_t<twk::COUNT_NW>)); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms,e0,e1)); if(i>=3&&ms<best)best=ms; }
      ms_all.push_back(best);
    }
    float mn=1e30f,mx=0; for(float x:ms_all){ mn=std::min(mn,x); mx=std::max(mx,x); }
    printf("R=%u W=%u, rows at %d offsets of %zu bytes: best launch %.3f .. %.3f ms (ratio %.2f)\n  ",R,W,n,step,mn,mx,mx/mn);
    for(int o=0;o<n;++o) printf("%.2f%s",ms_all[o],(o%16==15)?"\n  ":" "); printf("\n");
    return 0;
  }
  if(getenv("FINISH")){   // probe: per-block finish times of the static list kernel (2 full rounds), by XCD
    const twk::CountTable tb=make_table(R,W,0,true,P,min_chunks,dt,true);
    const twk::CountWork w=twk::count_work(d,W,0,0,dt,tb,C,R,tick,0,nullptr);
    const int probe_reps = getenv("FINISH_REPS")? atoi(getenv("FINISH_REPS")) : 2;       // launches back to back; the last one is reported
    for(int rep=0;rep<probe_reps;++rep){ CK(hipMemset(tick,0,4)); CK(twk::enqueue_count(0,w,tb,P,128u,nullptr,twk::k_count_list_t<twk::COUNT_NW,5>)); }
    CK(hipDeviceSynchronize());
    std::vector<unsigned long long> o4(4*P); CK(hipMemcpy(o4.data(),C,o4.size()*8,hipMemcpyDeviceToHost));
    std::vector<unsigned long long> o(2*P); for(uint32_t b=0;b<P;++b){ o[2*b]=o4[4*b]; o[2*b+1]=o4[4*b+1]; }
    { // the shader clock the blocks ran at: s_memtime ticks per tick of the constant 100 MHz counter, over each block's life
      double mn=1e30,mx=0,sum=0,life=0; for(uint32_t b=0;b<P;++b){ const double f=(double)o4[4*b+3]/(double)o4[4*b+2]*100.0; mn=std::min(mn,f); mx=std::max(mx,f); sum+=f; life+=o4[4*b+2]/100.0; }
      printf("shader clock over the blocks' lives (R=%u W=%u, second of two launches): mean %.0f MHz (min %.0f, max %.0f); mean block life %.1f us\n",R,W,sum/P,mn,mx,life/P); }
    unsigned long long t0=~0ull,t1=0; for(uint32_t b=0;b<P;++b){ t0=std::min(t0,o[2*b]); t1=std::max(t1,o[2*b]); }
    printf("finish-time spread over %u blocks: %.1f us (wall_clock64 ticks at 100 MHz)\n",P,(t1-t0)/100.0);
    for(int x=0;x<8;++x){ double mn=1e30,mx=0,sum=0; int n=0; for(uint32_t b=0;b<P;++b) if((int)(o[2*b+1]>>32&15)==x){ double t=(o[2*b]-t0)/100.0; mn=std::min(mn,t); mx=std::max(mx,t); sum+=t; ++n; }
      printf("  XCD %d: %3d blocks, finish offset min %.1f mean %.1f max %.1f us\n",x,n,mn,n?sum/n:0,mx); }
    // same-CU pairs
    printf("  first 16 blocks: "); for(uint32_t b=0;b<16;++b) printf("[b%u xcc%llu hw%05llx t%.0f] ",b,o[2*b+1]>>32&15,o[2*b+1]&0xFFFFF,(o[2*b]-t0)/100.0); printf("\n");
    return 0;
  }
  if(getenv("FUSED")){   // the fused count -> screen kernels on whole tiles (short rows), with their epilogue and without it (EXPERIMENT 6):
    // what does the screen cost next to the K loop?  Random rows, so nothing passes the screen.  LIVE=<words>: the row's live words (last chunk cut short)
    const uint32_t live = getenv("LIVE")? atoi(getenv("LIVE")) : W;
    const twk::CountTable tb=make_table(R,W,0,true,P,min_chunks,dt,false,true);
    const twk::CountWork w=twk::count_work(d,W,0,0,dt,tb,C,R,tick,twk::count_last_halves(live,W),nullptr);
    std::vector<uint32_t> pop(R+256); for(uint32_t r=0;r<R;++r){ uint32_t c=0; for(uint32_t k=0;k<W;++k) c+=__builtin_popcount(h[(size_t)r*W+k]); pop[r]=c; }
    uint32_t* dpop; CK(hipMalloc(&dpop,pop.size()*4)); CK(hipMemcpy(dpop,pop.data(),pop.size()*4,hipMemcpyHostToDevice));
    unsigned long long* dn; CK(hipMalloc(&dn,64)); CK(hipMemset(dn,0,64));
    twk::ScreenWork sw{}; sw.rowpop=dpop; sw.a0=0; sw.b0=0; sw.n_variants=R; sw.diag=0; sw.col_hi=nullptr; sw.list_zone=0; sw.probe_zone=0; sw.cut=0.1*(1.0-1e-6);
    sw.cand=C; sw.cap=(unsigned long long)R*R/8; sw.n_cand=dn; sw.chunk=64;
    twk::ScreenWork* dsw; CK(hipMalloc(&dsw,sizeof(sw)));
    float4* dterms; CK(hipMalloc(&dterms,(size_t)(R+256)*sizeof(float4)));
    const double tiles=(double)tb.n_tiles();
    for(int form=0; form<3; ++form){   // 0 phased (rows = variants), 1 unphased four products, 2 unphased three products (rows 2v, 2v+1 = H, Q)
      sw.nA=sw.nB= form? R/2 : R; sw.n_variants=sw.nA; sw.two_n = form? 2.0*W*32 : 1.0*W*32;
      hipLaunchKernelGGL(twk::k_screen_terms,dim3((sw.nA+255)/256),dim3(256),0,0,(const uint32_t*)dpop,sw.nA,form?2:1,sw.two_n,sw.cut,dterms);
      sw.terms=dterms; sw.slack=0.5f+(float)sw.two_n*(1.0f/1048576.0f);
      CK(hipMemcpy(dsw,&sw,sizeof(sw),hipMemcpyHostToDevice));
      for(int noepi=0; noepi<2; ++noepi){
        auto launch=[&](){ CK(hipMemsetAsync(tick,0,4,0)); CK(hipMemsetAsync(dn,0,8,0));
          void (*k)(twk::CountWork,const twk::ScreenWork*) =
            form==0? (noepi? twk::k_count_screen_t<twk::COUNT_NW,6> : twk::k_count_screen_t<twk::COUNT_NW,0>) :
            form==1? (noepi? twk::k_count_screen_unphased_t<twk::COUNT_NW,6> : twk::k_count_screen_unphased_t<twk::COUNT_NW,0>) :
                     (noepi? twk::k_count3_screen_unphased_t<twk::COUNT_NW,6> : twk::k_count3_screen_unphased_t<twk::COUNT_NW,0>);
          CK(twk::enqueue_count(0,w,tb,P,128u,nullptr,k,(const twk::ScreenWork*)dsw)); };
        launch(); launch(); CK(hipDeviceSynchronize());
        float best=1e30f;
        for(int i=0;i<reps;++i){ CK(hipEventRecord(e0)); launch(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms,e0,e1)); if(ms<best)best=ms; }
        unsigned long long nc=0; CK(hipMemcpy(&nc,dn,8,hipMemcpyDeviceToHost));
        const uint32_t words_done = w.last_halves? (W/twk::KC-1)*twk::KC + 2*w.last_halves : W;
        const double prod = tiles*128*128*words_done*(form==2?0.75:1.0), equiv = prod;
        printf("fused %-22s %-12s R=%u W=%u live=%u tiles=%.0f best %.3f ms  products/s %.3e  (%.1f%% of the and+bcnt ceiling 2.62e13)  candidates %llu\n",
               form==0?"phased":form==1?"unphased four-product":"unphased three-product", noepi?"no epilogue":"with screen", R,W,live,tiles,best,prod/best*1e3,equiv/best*1e3/2.6214e13*100,nc);
      }
    }
    return 0;
  }
  if(getenv("THREE")){   // the three-product form of the unphased planes (rows 2v / 2v + 1 = H / Q of variant v): k_count3_list_t against k_count_list_t on
    // the same rows, patch order, rectangle; checked against the host on sampled variant pairs
    const twk::CountTable tb=make_table(R,W,0,true,P,min_chunks,dt);
    const twk::CountWork w=twk::count_work(d,W,0,0,dt,tb,C,R,tick,0,nullptr);
    const double tiles=(double)tb.n_tiles(), wordops=tiles*128*128*W;
    if(const char* ex=getenv("EXPER")){   // timing only (wrong counts): the three- and four-product list kernels without the chunk barrier (7) / without the operand staging (8)
      const int which=atoi(ex);
      for(int three=0; three<2; ++three){
        auto launch=[&](){ CK(hipMemsetAsync(tick,0,4,0));
          void (*k)(twk::CountWork) = which==7? (three? twk::k_count3_list_t<twk::COUNT_NW,7> : twk::k_count_list_t<twk::COUNT_NW,7>) : (three? twk::k_count3_list_t<twk::COUNT_NW,8> : twk::k_count_list_t<twk::COUNT_NW,8>);
          CK(twk::enqueue_count(0,w,tb,P,three?64u:128u,nullptr,k)); };
        launch(); CK(hipDeviceSynchronize()); float best=1e30f;
        for(int i=0;i<reps;++i){ CK(hipEventRecord(e0)); launch(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms,e0,e1)); if(ms<best)best=ms; }
        const double exec=three? wordops*0.75 : wordops;
        printf("EXPERIMENT %d %-13s best %.3f ms  executed word-pairs/s %.3e (%.1f%% of the and+bcnt ceiling)\n",which,three?"three-product":"four-product",best,exec/best*1e3,exec/best*1e3/2.6214e13*100);
      }
      return 0;
    }
    // (form 2: the (U, Z) form - U = popc(H_A | H_B), Z = popc((Q_A ^ Q_B) & ~(H_A | H_B)) in the same matrix, two popcounts a word: 12 issue cycles where
    // the three products are 18; its percentage is of ITS ceiling, 1.31e13 pair-words/s.  ONLYFORM=<form>: that kernel alone, for counter passes)
    const int only_form = getenv("ONLYFORM")? atoi(getenv("ONLYFORM")) : -1;
    float best_of[3]={0,0,0};
    for(int three=0; three<3; ++three){
      if(only_form>=0 && three!=only_form) continue;
      auto launch=[&](){ CK(hipMemsetAsync(tick,0,4,0));
        void (*k)(twk::CountWork) = three==2? twk::k_count3_uz_list_t<twk::COUNT_NW> : three? twk::k_count3_list_t<twk::COUNT_NW> : twk::k_count_list_t<twk::COUNT_NW>;
        CK(twk::enqueue_count(0,w,tb,P,three?64u:128u,nullptr,k)); };
      CK(hipMemset(C,0xff,(size_t)R*R*4)); launch(); CK(hipDeviceSynchronize());
      if(three){ std::vector<uint32_t> hc((size_t)R*R/2); CK(hipMemcpy(hc.data(),C,hc.size()*4,hipMemcpyDeviceToHost)); int bad=0; std::mt19937 r2(7);
        for(int s=0;s<2000;++s){ const uint32_t a=r2()%(R/2), b=r2()%(R/2); uint32_t hh=0, ss=0;
          for(uint32_t k=0;k<W;++k){ const uint32_t ha=h[(size_t)(2*a)*W+k], qa=h[(size_t)(2*a+1)*W+k], hb=h[(size_t)(2*b)*W+k], qb=h[(size_t)(2*b+1)*W+k];
            if(three==2){ hh+=__builtin_popcount(ha|hb); ss+=__builtin_popcount((qa^qb)&~(ha|hb)); }
            else { hh+=__builtin_popcount(ha&hb); ss+=__builtin_popcount(qa&(hb|qb))+__builtin_popcount((ha|qa)&qb); } }
          const uint32_t g0=hc[(size_t)a*R+2*b], g1=hc[(size_t)a*R+2*b+1];
          if(g0!=hh||g1!=ss){ if(bad<5) printf("MISMATCH %s (%u,%u) ref %u %u got %u %u\n",three==2?"uz":"three",a,b,hh,ss,g0,g1); ++bad; } }
        printf("check %s: %d mismatches\n",three==2?"uz":"three-product",bad); bad_total+=bad; }
      else check("four-product",0);
      float best=1e30f;
      for(int i=0;i<reps;++i){ CK(hipEventRecord(e0)); launch(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms,e0,e1)); if(ms<best)best=ms; }
      best_of[three]=best;
      const double exec=three==2? wordops*0.25 : three? wordops*0.75 : wordops, ceiling=three==2? 1.3107e13 : 2.6214e13;
      printf("%-13s R=%u W=%u P=%u tiles=%.0f whole=%u units=%u best %.3f ms  variant pairs/s %.4e  executed %s/s %.3e (%.1f%% of the %s ceiling %.3g)\n",
             three==2?"uz":three?"three-product":"four-product",R,W,P,tiles,tb.first_split,w.n_units,best,tiles*64*64/best*1e3,three==2?"pair-words":"word-pairs",exec/best*1e3,exec/best*1e3/ceiling*100,
             three==2?"or+bcnt+bitop3+bcnt":"and+bcnt",ceiling);
    }
    if(best_of[1]>0 && best_of[2]>0) printf("uz / three-product: %.4f\n",best_of[2]/best_of[1]);
    return bad_total!=0;
  }
  const int only_mode = getenv("ONLYMODE")? atoi(getenv("ONLYMODE")) : -1;     // counter passes: one kernel form (2 = list/patch), rectangle only
  for(int diag=0; diag<(only_mode>=0?1:2); ++diag){
    double tiles = diag? (double)(R/128)*(R/128+1)/2 : (double)(R/128)*(R/128);
    double wordops = tiles*128*128*W;
    for(int mode=0; mode<3; ++mode){     // 0 grid, 1 list row-major, 2 list patch order, 3.. timing probes
      if(only_mode>=0 && mode!=only_mode) continue;
      const twk::CountTable tb = mode? make_table(R,W,diag,mode>=2,P,min_chunks,dt,true) : twk::CountTable();
      const twk::CountWork w=twk::count_work(d,W,0,0,dt,tb,C,R,tick,0,nullptr);
      auto launch=[&](){
        if(!mode){ hipLaunchKernelGGL((twk::k_count_tile_t<twk::COUNT_NW>),grid,block,0,0,d,W,0u,0u,diag,C,R); return; }
        CK(hipMemsetAsync(tick,0,4,0));
        CK(twk::enqueue_count(0,w,tb,P,128u,nullptr,getenv("NOSTORE")? twk::k_count_list_t<twk::COUNT_NW,6> : twk::k_count_list_t<twk::COUNT_NW>));
      };
      static const char* names[]={"grid","list","list/patch"};
      CK(hipMemset(C,0xff,(size_t)R*R*4));
      launch(); CK(hipDeviceSynchronize());
      check(names[mode],diag);
      float best=1e30f;
      for(int i=0;i<reps;++i){ CK(hipEventRecord(e0)); launch(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms,e0,e1)); if(ms<best)best=ms; }
      printf("%-10s diag=%d R=%u W=%u P=%u tiles=%.0f whole=%u units=%u best %.3f ms  word-pairs/s %.3e  VALU lane-ops/s %.3e (%.1f%% of 7.86e13; %.1f%% of the and+bcnt ceiling 2.62e13)\n",
             names[mode],diag,R,W,P,tiles,mode?tb.first_split:0u,mode?w.n_units:0u,best,wordops/best*1e3,2*wordops/best*1e3,2*wordops/best*1e3/7.864e13*100,wordops/best*1e3/2.6214e13*100);
    }
  }
  return bad_total!=0;
}
