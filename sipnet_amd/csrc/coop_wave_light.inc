// coop_wave_light.inc -- wave L: potential photosynthesis (canopy layers), the factors where there is no wave F
// Part of coopBody (step_coop.hip), #included INSIDE that function where the code used to stand (one kernel function, one
// branch per role: see the map in step_coop.hip).  From the enclosing scope: a (FastArgs), the template parameters, lane, col, nc,
// PRM / ST, tBegin, tEnd, act, live, EC, stageTile / tileFirst, the hand-over primitives.
// INTERFACE (mailboxes of coop_mailboxes.inc; "(t)" = the step the value belongs to)
//   takes   mailLai / seqLai          lai(t) from wave C (speculative until C's alive word confirms it: the value is used at once)
//           seqMinN (nitrogen-cycle layouts: progress only -- its factor rows are re-used once S is past them)
//   posts   mailPgp / seqPgp          potential gross photosynthesis + base foliar respiration of step t  -> wave W
//           mailFac rows 0..4 / seqFac   g1 g2 qSoilT gFine gCoarse of step t + 1 (layouts without a wave F)     -> wave C (and S)
//   side job: sipnet_batch_run_stats on the layouts without a wave F (coop_stats.inc)

  // =============================================================================================
  if (role == 2) {
    // Every layout of this wave must produce the same bits (they are tested against each other),
    // and what fuses into an FMA under -ffp-contract=fast depends on which neighbouring
    // expressions share a product (the factor block is here in some layouts and on wave F in
    // others): so no implicit fusion in this wave, constants included; the FMAs that matter are
    // written out below
#pragma clang fp contract(off)
    COOP_CODE_PHASE(2);
    if constexpr (kCoopCarriedTile<R, PlainExp, RingLds, Full, NP, NCyc, Ext, Sums>) COOP_CARRIED_PAD(7);   // (see coopCarriedPad)
    // ---- L: potPsn() + calcLightEff(), sipnet.c:517-641 -------------------------------------
    const double leafCSpWt = PRM(leafCSpWt);
    const double convK = kCWeight * (1.0 / kTen9) * (leafCSpWt / PRM(cFracLeaf)) * kSecPerDay;
    const double respPerGram = PRM(baseFolRespFrac) * PRM(aMax);
    const R K_g = (R)((PRM(aMax) * PRM(aMaxFrac) + respPerGram) * convK);
    const R K_tmin = (R)PRM(psnTMin), K_tmax = (R)PRM(psnTMax);
    const R K_invDen = (R)(1.0 / (((PRM(psnTMax) - PRM(psnTMin)) / 2.0) * ((PRM(psnTMax) - PRM(psnTMin)) / 2.0)));
    const R K_slope = (R)PRM(dVpdSlope), K_vexp = (R)PRM(dVpdExp);
    const R K_attl = (R)(-PRM(attenuation) * (1.0 / 6.0) * kLog2e);
    const R K_invHalf = (R)(1.0 / PRM(halfSatPar));
    // for wave C's respiration terms: everything that depends on climate and parameters only
    const R K_frozThr = (R)PRM(frozenSoilThreshold);
    const R K_lgVeg = (R)log2(PRM(vegRespQ10)), K_lgSoil = (R)log2(PRM(soilRespQ10));
    const R K_lgFine = (R)log2(PRM(fineRootQ10)), K_lgCoarse = (R)log2(PRM(coarseRootQ10));
    const R K_fol = (R)((PRM(baseFolRespFrac) * PRM(aMax)) *
                        (kCWeight * (1.0 / kTen9) * (PRM(leafCSpWt) / PRM(cFracLeaf)) * kSecPerDay) *
                        (1.0 / PRM(leafCSpWt)) * exp2(-(PRM(psnTOpt) / 10.0) * log2(PRM(vegRespQ10))));
    const R K_frozFolEff = (R)PRM(frozenSoilFolREff);
    const R K_bvr = (R)PRM(baseVegResp), K_bsr = (R)PRM(baseSoilResp);
    const R K_bfr = (R)PRM(baseFineRootResp), K_bcr = (R)PRM(baseCoarseRootResp);
    R qSoil = 0, gFine = 0, gCoarse = 0;
    bool haveQ = false;
    WAIT_DECL()
    // Every parameter load above has landed before the loop starts, and the compiler is told so (a
    // wait it can see): its wait-count bookkeeping would otherwise put a full `s_waitcnt vmcnt(0)` in
    // front of the first in-loop use of each of these constants -- in the middle of the day step, where
    // it would sit out the statistics loads (and the tile DMA) on every iteration
    __builtin_amdgcn_s_waitcnt(0);
    for (int tileStart = curTile * kFastTile; tileStart < tEnd; tileStart += kFastTile, curTile++) {
      if (tileStart > tBegin) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // DMA of 16 steps ago
      stageTile(curTile + 1, (curTile + 1) & 1);
      const int tFirst = tileStart > tBegin ? tileStart : tBegin;
      const int tLast = (tileStart + kFastTile) < tEnd ? (tileStart + kFastTile) : tEnd;
      const unsigned char* recB = lds + (curTile & 1) * kTileBytes +
                                  (int)(tFirst - tileFirst(curTile)) * (int)sizeof(FastRec);
      for (int t = tFirst; t < tLast; t++, recB += sizeof(FastRec)) {
        d2 q1, q2, q3, q5;
        double q6x;
        int bitsV;
        asm volatile("ds_read_b32 %0, %6 offset:128\n\tds_read_b128 %1, %6 offset:16\n\t"
                     "ds_read_b128 %2, %6 offset:32\n\tds_read_b128 %3, %6 offset:48\n\t"
                     "ds_read_b128 %4, %6 offset:80\n\tds_read_b64 %5, %6 offset:96\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(bitsV), "=&v"(q1), "=&v"(q2), "=&v"(q3), "=&v"(q5), "=&v"(q6x)
                     : "v"(ldsAddr(recB)) : "memory");
        const int bits = uni(bitsV);
#ifdef SIPNET_COOP_BOUNDED
        // the error path's own test (SIPNET_KOPT_WAIT_SELFTEST): this wave stops posting after 100 steps, the others'
        // waits must give up and the launch must end with the report
        if ((a.options & SIPNET_KOPT_WAIT_SELFTEST) && t == tBegin + 100) return;
#endif
        if (!Staged && statsHere && t == statNext) statAct(false);
        // ---- for wave C: the climate / parameter part of its respiration terms of THIS step
        // (vegResp sipnet.c:1051-1068, calcRootResp :1073, calcSoilRespiration :1132-1148 with
        // depeffects.c:71-74):  folResp = leafC * g1,  rVeg = folResp + totalWoodC * g2,
        // rSoil = soilC * (qSoilT * moistEff[wave W]),  rFineRoot = fineRootC * gFine,
        // rCoarseRoot = coarseRootC * gCoarse.  Nothing here depends on member state, so this
        // wave -- idle at night and while it waits for the leaf area by day -- runs it ahead of
        // C: the slot of step t was last used for step t-2, which C is past once it has posted
        // the leaf area of step t-1
        if (!FacWave) {  // (wave F's job when there is one)
          WAIT_BEGIN()
          awaitAtLeast(&seqLai, t - 1);
          // NCyc: wave S reads two rows of the block too, at the start of ITS step -- which C's progress
          // does not vouch for (C(t-1) only needs S's nitrogen block of step t-2 done): the slot is free
          // once S has posted the mineral nitrogen of step t-1, which it does after that read (found by the fuzzer:
          // one trial in 600 had S take the soil factors of step t+2 for step t, 2e-5 off on NEE)
          if (NCyc) awaitAtLeast(&seqMinN, t - 1);
          WAIT_END(1)
          const R vegQ = fexp2(q10Arg(recR<R>(q5.y), K_lgVeg), EC);
          R g1 = K_fol * vegQ;
          g1 = (recR<R>(q1.y) < K_frozThr) ? g1 * K_frozFolEff : g1;
          const R g2 = K_bvr * vegQ;
          if (!haveQ || !(bits & FAST_TSOIL_SAME)) {
            const R tsoil10 = recR<R>(q6x);
            qSoil = fexp2(q10Arg(tsoil10, K_lgSoil), EC);
            gFine = K_bfr * fexp2(q10Arg(tsoil10, K_lgFine), EC);
            gCoarse = K_bcr * fexp2(q10Arg(tsoil10, K_lgCoarse), EC);
            haveQ = true;
          }
          const R qSoilT = K_bsr * qSoil * recR<R>(q3.x);
          if (NCyc) postRaw(&mailFac[t & 1][6][lane], qSoil);   // before the flag post5 sets
          post5(&mailFac[t & 1][0][lane], &seqFac, g1, g2, qSoilT, gFine, gCoarse, t);
        }
        // (staged statistics: after the factor post, so that C has what it waits for.  C and W cannot be back
        // at the half's rows before this wave is done with them: they are kStageR - 1 steps away from it when
        // the action starts, and by day they need this wave's potential photosynthesis to go on)
        // (round 5 moved this to the factor wave of the two-chunk layout -- it shares its SIMD with a water wave, the
        // light wave with the other chunk's carbon wave -- and measured nothing: c4 run_stats 12.0 -> 11.9 ms.  What the
        // staged statistics cost there, 1.7 ms, is C's and W's own stage writes, not where the half is summed.)
        if (Staged && stageOn && t == statNext) stagedAct();
        if (!(bits & FAST_PAR_POS)) continue;  // night: potGrossPsn = 0, nobody waits for it
        {
        const R tair = recR<R>(q1.x);
        // climate-only factors first, then the leaf area of this step
        const R dTemp = rmax0((K_tmax - tair) * (tair - K_tmin) * K_invDen);
        R vpdPow = recR<R>(q2.y) * recR<R>(q2.y);
        if (!PlainExp)
          vpdPow = (K_vexp == R(2)) ? vpdPow : fexp2(K_vexp * recR<R>(((const double*)(recB + 144))[2]), EC);
        const R dVpd = rmax0(ffma(-K_slope, vpdPow, R(1)));
        const R q = recR<R>(q2.x) * K_invHalf;
        const R e0 = fexp2(q, EC);
        WAIT_BEGIN()
        const R lai = take(&mailLai[t & 1][lane], &seqLai, t);
        WAIT_END(0)
        const R r1 = fexp2(K_attl * lai, EC);
        const R r2 = r1 * r1, r3 = r2 * r1, r4 = r2 * r2, r5 = r4 * r1, r6 = r3 * r3;
        const R e1 = fexp2(q * r1, EC), e2 = fexp2(q * r2, EC), e3 = fexp2(q * r3, EC);
        const R e4 = fexp2(q * r4, EC), e5 = fexp2(q * r5, EC), e6 = fexp2(q * r6, EC);
        const R s = ffma(R(2), e2 + e4, ffma(R(4), (e1 + e3) + e5, e0 + e6));
        const R dLight = ffma(-s, R(1.0 / 18.0), R(1));
        post(&mailPgp[t & 1][lane], &seqPgp, K_g * lai * dTemp * dVpd * dLight, t);
        }
      }
    }
    WAIT_STORE(0)
    if (Staged && stageOn) stagedFinish();
    else if (statsHere) statFinish();
    return;
  }
