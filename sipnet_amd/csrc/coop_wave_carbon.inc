// coop_wave_carbon.inc -- wave C: carbon fluxes, pools, phenology, mortality, the running mean, NEE
// Part of coopBody (step_coop.hip), #included INSIDE that function where the code used to stand (one kernel function, one
// branch per role: see the map in step_coop.hip).  From the enclosing scope: a (FastArgs), the template parameters, lane, col, nc,
// PRM / ST, tBegin, tEnd, act, live, EC, stageTile / tileFirst, the hand-over primitives.
// INTERFACE
//   takes   mailFac rows 0..6 / seqFac, seqMoist   the step's factors (one round trip with the record; regular tiles: no record at all)
//           mailPsn / seqPsn          photosynthesis of step t from wave W (after lai(t + 1) has been posted: off the critical path)
//           nitrogen-cycle layouts: mailMinN / seqMinN (looked at in the factor take, waited for after the own posts), mailSupply /
//           seqSupply (a nitrogen-limited step only), mailStorN / seqStorN (leaf-on events; PairDiag: S's "through with the step before")
//   posts   mailLai / seqLai, mailAlive   lai(t + 1) BEFORE waiting for photosynthesis(t), confirmed or revoked after the mortality test
//                                                                                                               -> waves L, W
//           nitrogen-cycle layouts: mailPlant / seqPlant (litter fluxes, N demand: early), mailEvent / seqEvent, mailDemand /
//           seqDemand, mailDeath, mailPend (GPP - R_a [+ R_a, root respiration; + the mass totals: diagnostics]) then the verdict
//           word                                                                                                -> wave S
//   stores  the NEE plane (or its sums; not on the nitrogen-cycle layouts: S forms NEE), plant pools, ring, accumulators, record

  // =============================================================================================
  // ---- C: carbon fluxes, pools, trackers, running mean (sipnet.c:756-842, 1051-1196, 1420-1806)
  COOP_CODE_PHASE(0);
  constexpr bool Carried = kCoopCarriedTile<R, PlainExp, RingLds, Full, NP, NCyc, Ext, Sums>;
  const R K_invLcsw = (R)(1.0 / PRM(leafCSpWt));
  const R K_wtr = (R)PRM(woodTurnoverRate), K_ltr = (R)PRM(leafTurnoverRate);
  const R K_frt = (R)PRM(fineRootTurnoverRate), K_crt = (R)PRM(coarseRootTurnoverRate);
  const R K_la = (R)PRM(leafAllocation), K_wa = (R)PRM(woodAllocation);
  const R K_fa = (R)PRM(fineRootAllocation), K_ca = (R)PRM(coarseRootAllocation);
  // leaf-on threshold of the variable the plan put into the record: year-to-date GDD -- or, with the gdd flag
  // off, soil temperature / day of year, whose threshold convertParamsKernel has then put into this row
  // (choosing among the three parameters here, by flag or by a row index from the host, cost the
  // one-chunk kernel 0.6 - 3 %: register allocation, not work)
  const double gddLeafOn = PRM(gddLeafOn);
  const double leafOffDay = PRM(leafOffDay) > 0 ? PRM(leafOffDay) : 1e300;

  // NCyc: reciprocal C:N ratios for the plants' nitrogen demand (nitrogen.c:89-104) and the test both
  // waves make (nPlentiful); soil carbon lives on wave W then
  const R G_iLeafCN = NCyc ? (R)(1.0 / PRM(leafCN)) : R(0), G_iWoodCN = NCyc ? (R)(1.0 / PRM(woodCN)) : R(0);
  const R G_iFineCN = NCyc ? (R)(1.0 / PRM(fineRootCN)) : R(0), G_resorbC = NCyc ? (R)PRM(leafNResorptionFrac) : R(0);
  const double G_nVolD = NCyc ? PRM(nVolatilizationFrac) : 0.0, G_nLeachD = NCyc ? PRM(nLeachingFrac) : 0.0;
  double plantWoodC = ST(plantWoodC), plantLeafC = ST(plantLeafC), soilC = NCyc ? 0.0 : ST(soilC);
  double coarseRootC = ST(coarseRootC), fineRootC = ST(fineRootC);
  // Ext: growth respiration; Opt: the litter pool, methane and carbon saturation on this wave (rates 0 / share 0
  // with their flags off: the same few instructions run to an exactly unchanged result)
  const R X_growthFrac = F_growthResp ? (R)PRM(growthRespFrac) : R(0);
  const R X_lbrK = F_litterPool ? (R)(PRM(litterBreakdownRate) / PRM(baseSoilResp)) : R(0);
  const R X_flr = Opt ? (R)PRM(fracLitterRespired) : R(0), X_1mFlr = Opt ? (R)(1.0 - PRM(fracLitterRespired)) : R(0);
  const R X_soilCH4 = F_anaerobic ? (R)PRM(soilMethaneRate) : R(0);
  const R X_litCH4 = (F_anaerobic && F_litterPool) ? (R)PRM(litterMethaneRate) : R(0);
  const R X_iSoilCSat = (Opt && F_carbonSat) ? (R)(1.0 / PRM(soilCSaturation)) : R(0);
  double litterC = Opt ? ST(litterC) : 0.0;
  // the soil side of a step with the optional pools (Opt), ONE piece of code for the regular-tile path and the
  // general step (a wavefront's path depends on its neighbours: same bits): calcSoilRespiration / calcLitterFluxes /
  // calcMethaneFlux (sipnet.c:1132-1214) and updatePoolsForSoil (sipnet.c:1645-1668, both forms, one select).
  // soilCNow: the soil carbon the reference looks at for the saturation share -- it already holds the step's events.
  auto optSoilSide = [&](R eSoilC, R eLitter, R soilCNow, R fSoil, R qSoilT, R mK, R rootLoss, R aboveLitter, R len,
                         R& rSoil, R& rHet, double& soilGain, double& litterGain, R& methane) {
#pragma clang fp contract(off)
    rSoil = eSoilC * fSoil;
    const R breakdown = eLitter * (X_lbrK * fSoil);
    const R rLitter = breakdown * X_flr, litterToSoil = breakdown * X_1mFlr;
    const R qm = qSoilT * mK;
    const R soilMethane = X_soilCH4 * eSoilC * qm, litterMethane = X_litCH4 * eLitter * qm;
    const R sat = clip01(soilCNow * X_iSoilCSat);          // 0 without carbon saturation
    const R soilInputs = rootLoss + litterToSoil;
    const R dLitter = aboveLitter + soilInputs * sat - litterToSoil - rLitter - litterMethane;
    const R dSoilTwo = soilInputs * (R(1) - sat) - rSoil - soilMethane;
    const R dSoilOne = rootLoss + aboveLitter - rSoil - soilMethane;
    soilGain = (double)((F_litterPool ? dSoilTwo : dSoilOne) * len);
    litterGain = (double)((F_litterPool ? dLitter : R(0)) * len);
    rHet = rSoil + rLitter;
    methane = soilMethane + litterMethane;   // (Full: record column 31, and the carbon balance)
  };
  double delta = ST(plantCAccountingDelta);
  double ringSum = ST(ringSum), totNee = ST(totNee);
  int phenBits = (int)ST(phenBits);
  int ringValidFrom = (int)ST(ringValidFrom);
  int diedAt = (int)ST(diedAt);
  // Full: the other accumulators of updateTrackers(), the record's constant columns (pools the
  // default flag set never touches) and the diagnostics counters
  double totRtot = Full ? ST(totRtot) : 0.0, totRa = Full ? ST(totRa) : 0.0;
  double totRh = Full ? ST(totRh) : 0.0, totNpp = Full ? ST(totNpp) : 0.0;
  double yGpp = Full ? ST(yearlyGpp) : 0.0, yRtot = Full ? ST(yearlyRtot) : 0.0;
  double yRa = Full ? ST(yearlyRa) : 0.0, yRh = Full ? ST(yearlyRh) : 0.0;
  double yNpp = Full ? ST(yearlyNpp) : 0.0, yNee = Full ? ST(yearlyNee) : 0.0;
  double yLitter = Full ? ST(yearlyLitter) : 0.0;
  const double cLitterC = Full ? ST(litterC) : 0.0, cMinN = Full ? ST(minN) : 0.0;
  const double cSoilOrgN = Full ? ST(soilOrgN) : 0.0, cLitterN = Full ? ST(litterN) : 0.0;
  const double cStorN = Full ? ST(plantStorageN) : 0.0;
  const bool wantDiag = Full && !NCyc && a.diag != nullptr;
  // NCyc, one chunk per workgroup: the pools are spread over two wavefronts -- this one sends the plant side's totals to
  // wave S (mailPend rows 3 .. 13), which runs the balance check; the clamp warnings of the plant pools are counted here
  const bool wantDiagN = Full && NCyc && (NP == 1 || PairDiag) && a.diag != nullptr;
  int clampWarn = 0, balanceWarn = 0;
  double maxDC = 0.0;
  double* __restrict__ recp = Full && a.rec ? a.rec + col : nullptr;

  // the ring in HBM holds NPP values of type R (fp32-mixed batches: fp32 numbers, stored as such); the LDS copy is fp64
  R* __restrict__ ringp = (R*)a.ring + col;
  OutT* __restrict__ oNee = (OutT*)(a.nee ? a.nee : a.scratchRow) + col;
  const int64_t ldNee = a.nee ? a.ld : 0;
  const uint32_t ncu = (uint32_t)nc;
  CoopSums<Sums> sumsC;   // Sums: the group's sum so far, and the steps it still lacks
  if constexpr (Sums) sumsC.left = a.sumEvery;

  post(&mailLai[tBegin & 1][lane], &seqLai, (R)plantLeafC * K_invLcsw, tBegin);
  postAlive(&mailAlive[tBegin & 1][lane], tBegin, false);  // lai(tBegin) is not speculative
  // The two phenology switches fire once a year per member; whether ANY member of the wave can
  // fire in a step is decided with two wave-uniform compares against the smallest thresholds
  // of the wave, and not at all once every member has fired
  double minGddOn = gddLeafOn, minOffDay = leafOffDay;
  for (int off = 32; off > 0; off >>= 1) {
    minGddOn = fmin(minGddOn, __shfl_xor(minGddOn, off, 64));
    minOffDay = fmin(minOffDay, __shfl_xor(minOffDay, off, 64));
  }
  bool allOn = __builtin_amdgcn_ballot_w64((phenBits & 1) == 0) == 0;
  bool allOff = __builtin_amdgcn_ballot_w64((phenBits & 2) == 0) == 0;
  // carried: this member's alive flag (sipnet.c:1530-1544) and, for the whole wave, "every
  // member alive with an untouched ring epoch" (what the regular ring update needs)
  bool aliveC = (plantWoodC > kTiny) && (plantWoodC + delta > kTiny) && (fineRootC + coarseRootC > kTiny);
  bool ringClean = __builtin_amdgcn_ballot_w64(!aliveC || ringValidFrom > 0) == 0;
  if (RingLds) {
    for (int k = 0; k < SIPNET_RING_SLOTS; k++) ringL[k * 64 + lane] = (double)ringp[(uint32_t)k * ncu];
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  }
  WAIT_DECL()
  // HBM ring: the value written by the previous step is forwarded from a register
  double lastNpp = 0.0;
  int lastIns = -1;
  CSTAMP_DECL()

  // NCyc: what wave S needs of a step's plant side (the litter fluxes, the nitrogen demand of the creation
  // fluxes nitrogen.c:89-104, the resorption of a negative total creation :170-196, the leaf-on nitrogen
  // :84-86), posted as soon as the creation fluxes are known -- S is working on the soil side of the same
  // step -- and checkNitrogenLimitation() (limitations.c:69-114): both waves test "plentiful" with the
  // same numbers; only where it fails for some member does C wait for S's exact supply, scale its
  // creation fluxes and answer with the demand that is left
  auto plantSideN = [&](int t, R len, R invLen, double minNStep, int minNSeq, double qSoilD, double lenD, R leafLitter, R woodLitter,
                        R fineRootLoss, R coarseRootLoss, R leafOnCreation, R evLeafOnAll, R& leafCreation,
                        R& woodCreation, R& fineRootCreation, R& coarseRootCreation) {
#pragma clang fp contract(off)
    auto leafOnN = [&](R leafOnC) -> R { return rmax0(leafOnC * G_iLeafCN - leafOnC * G_iWoodCN); };
    auto plantNDemand = [&]() -> R {
      return rmax0(woodCreation * G_iWoodCN + leafCreation * G_iLeafCN + fineRootCreation * G_iFineCN +
                   coarseRootCreation * G_iWoodCN);
    };
    R reductionN = 0;
    if (woodCreation + leafCreation + fineRootCreation + coarseRootCreation < R(0))
      reductionN -= (leafCreation * G_iLeafCN + woodCreation * G_iWoodCN + coarseRootCreation * G_iWoodCN +
                     fineRootCreation * G_iFineCN);
    const R nDemand = plantNDemand();
    postD(&mailPlant[t & 1][0][lane], 0, (double)leafLitter);
    postD(&mailPlant[t & 1][0][lane], 1, (double)woodLitter);
    postD(&mailPlant[t & 1][0][lane], 2, (double)fineRootLoss);
    postD(&mailPlant[t & 1][0][lane], 3, (double)coarseRootLoss);
    postD(&mailPlant[t & 1][0][lane], 4, (double)nDemand);
    postD(&mailPlant[t & 1][0][lane], 5, (double)reductionN);
    postD(&mailPlant[t & 1][0][lane], 6, (double)leafOnN(leafOnCreation + evLeafOnAll));
    postD(&mailPlant[t & 1][0][lane], 7, (double)leafOnN(leafOnCreation));
    postFlag(&seqPlant, t);
    // S's mineral nitrogen of this step: normally it came with the factors; if S was not that far yet
    // it is waited for only NOW, after the post S itself is waiting for (C -> S -> C would otherwise be
    // one latency chain per step)
    if (__builtin_expect(minNSeq < t, 0)) {
      WAIT_BEGIN()
      takeD1(&mailMinN[t & 1][lane], &seqMinN, t, minNStep);
      WAIT_END(2)
    }
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!nPlentiful(minNStep, qSoilD, lenD, G_nVolD, G_nLeachD, (double)nDemand)) != 0, 0)) {
      double sAvail, sFixFrac, sUnclaimed;
      takeD3(&mailSupply[0][lane], &seqSupply, t, sAvail, sFixFrac, sUnclaimed);
      const R availableMinN = (R)sAvail, fixFrac = (R)sFixFrac, unclaimed = (R)sUnclaimed;
      const R nUptake = (R(1) - fixFrac) * rmax0(nDemand - unclaimed * invLen);
      const R uptakeDemand = nUptake * len;
      const bool limited = uptakeDemand > R(kTiny) && uptakeDemand > availableMinN;
      const R red = limited ? fdiv(fdiv(availableMinN, R(1) - fixFrac) + unclaimed, nDemand * len) : R(1);
      woodCreation *= red;
      leafCreation *= red;
      fineRootCreation *= red;
      coarseRootCreation *= red;
      postD(&mailDemand[0][lane], 0, (double)plantNDemand());
      postFlag(&seqDemand, t);
    }
  };

  if constexpr (Carried) COOP_CARRIED_PAD(0);
  for (int tileStart = curTile * kFastTile; tileStart < tEnd; tileStart += kFastTile, curTile++) {
    // the DMA of this tile was issued a tile ago; only the last step's two stores may still be
    // in flight behind it
    if constexpr (Sums) {   // (no NEE store per step: nothing, or the ring store alone, may stay in flight)
      if (tileStart > tBegin) {
        if (RingLds) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
      }
    } else {
    if (tileStart > tBegin) {
      if (RingLds) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");  // + the ring store
    }
    }
    stageTile(curTile + 1, (curTile + 1) & 1);
    const int tFirst = tileStart > tBegin ? tileStart : tBegin;
    const int tLast = (tileStart + kFastTile) < tEnd ? (tileStart + kFastTile) : tEnd;
    const unsigned char* recB = lds + (curTile & 1) * kTileBytes +
                                (int)(tFirst - tileFirst(curTile)) * (int)sizeof(FastRec);
    int t = tFirst;
    // ======== regular tile (plan.h, FastRec::tileBits) ==========================================
    // Every step of the tile has the same length and the same one or two ring evictions with all
    // slots advancing by one, no events, no year roll-over; and, for THIS wavefront, every member
    // is alive with an untouched ring epoch and no phenology switch can fire before the tile ends
    // (year-to-date GDD and the day of year only grow inside a tile).  Then the carbon block needs
    // no per-step record at all: step length and eviction weights are hoisted, the slots counted,
    // the day / night flags come from the tile's mask, and the oldest ring value is the one read
    // as "second eviction" the step before.  Same arithmetic as the general step below; left at
    // the first step on which a member dies.  (Lean instantiation only: records, all accumulators
    // and diagnostics take the general step.)
    if (!Full && ringClean && !(a.options & SIPNET_KOPT_NO_REGULAR_TILES)) {
      d2 h0, h7;
      i4 hj;
      double hW1, hEndGdd, hEndDay;
      int hTile;
      asm volatile("ds_read_b128 %0, %7\n\tds_read_b128 %1, %7 offset:112\n\tds_read_b128 %2, %7 offset:128\n\t"
                   "ds_read_b64 %3, %7 offset:144\n\tds_read_b32 %4, %7 offset:208\n\tds_read_b64 %5, %7 offset:216\n\t"
                   "ds_read_b64 %6, %7 offset:224\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(h0), "=&v"(h7), "=&v"(hj), "=&v"(hW1), "=&v"(hTile), "=&v"(hEndGdd), "=&v"(hEndDay)
                   : "v"(ldsAddr(recB)) : "memory");
      const int tileBits = uni(hTile);
      const bool phenSafe = (allOn || hEndGdd < minGddOn) && (allOff || hEndDay < minOffDay);
      if ((tileBits & FAST_TILE_REGULAR) && __builtin_amdgcn_ballot_w64(!phenSafe) == 0) {
        const R len = (R)h0.x, invLen = (R)h0.y;
        const int nOps = uni(hj.x) >> 16;
        const int slots0 = uni(hj.y);
        auto nextSlot = [](int s) { return s + 1 == SIPNET_RING_SLOTS ? 0 : s + 1; };
        // two evictions: the first one's value is the one read as second eviction a step earlier
        const double wA = nOps == 2 ? h7.y : 0.0, wB = nOps == 2 ? hW1 : h7.y;
        int readSlot = nOps == 2 ? ((slots0 >> 8) & 255) : (slots0 & 255);
        int insSlot = uni(hj.z);
        double vPrev = 0.0;
        if (nOps == 2) {
          const int s0 = slots0 & 255;
          if constexpr (Carried)   // (read and awaited by hand, like every DS access of the step: the compiler counts none of its own there)
            asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(vPrev) : "v"(ldsAddr(&ringL[s0 * 64 + lane])) : "memory");
          else
          vPrev = RingLds ? ringL[s0 * 64 + lane] : (s0 == lastIns ? lastNpp : (double)ringp[(uint32_t)s0 * ncu]);
        }
        // The rest of a step, written once and instantiated twice: the common case (nobody dies: no
        // mortality code at all behind ONE wave-uniform test) inside the loop, and the step on which a
        // member of the wavefront dies AFTER the loop, which that step leaves (the wavefront takes the
        // general step from then on) -- the loop body stays one straight run of code.  What the
        // tail needs from the step lives outside the loop for that.
        // Carried (kCoopCarriedTile, step_coop.hip: c10k's instantiation alone): what a step needs of t's parity and of the ring
        // slots is CARRIED from step to step as per-lane LDS byte addresses instead of being derived from t and the slot numbers
        // -- a two-slot mailbox's address flips with one subtraction from the sum of both slots' addresses, a ring address
        // advances by a slot's 512 bytes, the posted sequence number by one -- and re-seeded at the top of every regular tile.
        // The ring's wrap is a wave-uniform test against the step on which it falls (wrapNext), corrected out of line.
        [[maybe_unused]] unsigned cFac = 0, cLai = 0, cAlive = 0, cRead = 0, cIns = 0;   // mailFac[t & 1], mailLai / mailAlive[(t + 1) & 1], ringL[readSlot / insSlot]
        [[maybe_unused]] unsigned sumFac = 0, sumLai = 0, sumAlive = 0, sumPsnLai = 0;
        [[maybe_unused]] int cSeq = 0;                                                   // t + 1
        [[maybe_unused]] int wrapRead = 0, wrapIns = 0, wrapNext = 0;                    // the steps that use the ring's last slot
        [[maybe_unused]] uint64_t allLanes = 0;
        if constexpr (Carried) {
          cFac = ldsAddr(&mailFac[t & 1][0][lane]);
          sumFac = ldsAddr(&mailFac[0][0][lane]) + ldsAddr(&mailFac[1][0][lane]);
          cLai = ldsAddr(&mailLai[(t + 1) & 1][lane]);
          sumLai = ldsAddr(&mailLai[0][lane]) + ldsAddr(&mailLai[1][lane]);
          cAlive = ldsAddr(&mailAlive[(t + 1) & 1][lane]);
          sumAlive = ldsAddr(&mailAlive[0][lane]) + ldsAddr(&mailAlive[1][lane]);
          // mailPsn[t & 1] is the OTHER slot of the two (same stride as mailLai): this sum less cLai, on the day path only
          static_assert(sizeof(mailPsn[0]) == sizeof(mailLai[0]), "mailPsn[t & 1] from mailLai[(t + 1) & 1]: the same slot stride");
          sumPsnLai = ldsAddr(&mailPsn[1][lane]) + ldsAddr(&mailLai[0][lane]);
          cSeq = t + 1;
          asm volatile("" : "+v"(cSeq));   // (a vector register of its own: not t + 1 moved over every step)
          cRead = ldsAddr(&ringL[readSlot * 64 + lane]);
          cIns = ldsAddr(&ringL[insSlot * 64 + lane]);
          wrapRead = t + (SIPNET_RING_SLOTS - 1 - readSlot);
          wrapIns = t + (SIPNET_RING_SLOTS - 1 - insSlot);
          wrapNext = wrapRead < wrapIns ? wrapRead : wrapIns;
          allLanes = __builtin_amdgcn_ballot_w64(true);
        }
        R photosynthesis = 0, rSoil = 0, rVeg = 0, rCoarseRoot = 0, rFineRoot = 0, rHet = 0;
        [[maybe_unused]] R methaneReg = 0;
        double soilGain = 0.0, litterGain = 0.0, ringNew = 0.0;
        R rvN = 0;
        bool rootsOk = true, useLast = false, dyingStep = false;
        auto finishStep = [&](auto mayDie) {
#pragma clang fp contract(off)
          constexpr bool MayDie = decltype(mayDie)::value;
          bool diedNow = false;
          double deathToSoil0 = 0.0, deathToSoil1 = 0.0;
          // wave-uniform (this instantiation runs only when some member dies): the whole wavefront
          // takes the general step from now on -- a per-lane flag would send the survivors down the
          // regular tiles and the dead member down the general step of the SAME tile afterwards
          if (MayDie) ringClean = false;
          if (MayDie && !(rootsOk && (plantWoodC + delta > kTiny))) {  // every member was alive before
            aliveC = false;
            diedNow = true;
            if (diedAt < 0) diedAt = t;
            deathToSoil0 = fineRootC + coarseRootC;
            deathToSoil1 = plantWoodC + plantLeafC + delta;
            if (NCyc) {  // to wave S's pools (sipnet.c:1735-1746), before the verdict word that announces it
              postD(&mailDeath[0][lane], 0, deathToSoil0);
              postD(&mailDeath[0][lane], 1, deathToSoil1);
              postD(&mailDeath[0][lane], 2, fineRootC * (double)G_iFineCN + coarseRootC * (double)G_iWoodCN);
              postD(&mailDeath[0][lane], 3, plantWoodC * (double)G_iWoodCN + plantLeafC * (double)G_iLeafCN);
            }
            plantWoodC = 0.0;
            plantLeafC = 0.0;
            coarseRootC = 0.0;
            fineRootC = 0.0;
            delta = 0.0;
            ringSum = 0.0;
          }
          plantWoodC = rmax0(plantWoodC);
          plantLeafC = rmax0(plantLeafC);
          coarseRootC = rmax0(coarseRootC);
          fineRootC = rmax0(fineRootC);
          const R tGpp = photosynthesis * len;
          const R tRa = ffma(rVeg, len, (rCoarseRoot + rFineRoot) * len);
          if (NCyc) postD(&mailPend[t & 1][0][lane], 0, (double)(tGpp - tRa));   // S forms NEE (it has R_h); before the verdict word
          if constexpr (Carried) postAlive(ldsPtr<int>(cAlive), cSeq, diedNow);
          else postAlive(&mailAlive[(t + 1) & 1][lane], t + 1, diedNow);
          if (!NCyc) {
            soilC += soilGain;
            if (Opt) litterC += litterGain;
            if (MayDie && diedNow) {
              soilC += deathToSoil0;
              if (Opt && F_litterPool) litterC += deathToSoil1;   // sipnet.c:1735-1746: above-ground biomass to the litter pool
              else soilC += deathToSoil1;
            }
            soilC = rmax0(soilC);
            if (Opt) litterC = rmax0(litterC);
          }
          const R tRh = (Opt ? rHet : rSoil) * len;
          const R tNee = R(-1.0) * ((tGpp - tRa) - tRh);
          if (!NCyc) totNee += (double)tNee;
          const double npp = (double)(photosynthesis - rVeg - rCoarseRoot - rFineRoot);
          if (!RingLds) asm volatile("s_waitcnt vmcnt(0)" : "+v"(rvN) :: "memory");
          const double vNew = RingLds ? ringNew : (useLast ? lastNpp : (double)rvN);
          if (!(MayDie && diedNow)) {
            ringSum = ffma(-wA, vPrev, ringSum);
            ringSum = ffma(-wB, vNew, ringSum);
            ringSum = ffma(npp, (double)len, ringSum);
          } else {  // its ring epoch starts over; the other members carry on
            ringValidFrom = t + 1;
          }
          vPrev = vNew;
          if (RingLds) {
            if constexpr (Carried) postRaw(ldsPtr<double>(cIns), npp);   // (like the posts around it: no wait of the compiler's in the step)
            else ringL[insSlot * 64 + lane] = npp;
          } else {
            ringp[(uint32_t)insSlot * ncu] = (R)npp;   // (npp is an R-typed difference: nothing is lost)
            lastIns = insSlot;
            lastNpp = npp;
          }
          if constexpr (Sums && !NCyc) {   // (NCyc: wave S forms NEE, and sums it)
            sumsC.nee += (double)tNee;
            if (--sumsC.left == 0) {
              *oNee = (OutT)sumsC.nee;
              oNee += ldNee;
              sumsC.nee = 0.0;
              sumsC.left = a.sumEvery;
            }
          } else {
          if (!NCyc) {
            *oNee = tNee;
            oNee += ldNee;
          }
          }
          if (__builtin_expect(stageOn, 0)) postRaw(&stage[0][(t - tBegin) & (2 * kStageR - 1)][lane], tNee);
        };
        if constexpr (Carried) COOP_CARRIED_PAD(1);
        // (Carried: the mask stays where it is, step t's bit at position t & 31 -- nothing to shift along from step to step)
        unsigned dayMask = Carried ? ((unsigned)tileBits >> 16) << (tileStart & 16) : ((unsigned)tileBits >> 16) >> (t - tileStart);
        for (; t < tLast; t++, dayMask >>= Carried ? 0 : 1) {
          // The carbon wave's arithmetic is written out with explicit fused multiply-adds and
          // compiled with contraction off (here and in the general step below): which of the two
          // paths a wavefront takes depends on its 63 neighbours, so they must not differ by what
          // the compiler happens to fuse in one context and not in the other.
#pragma clang fp contract(off)
          MARK("C regular step begin")
          // this step's factors: five from wave F / L, the moisture effect from wave W (each flag read
          // before its values, one LDS round trip when both are current)
          R g1, g2, qSoilT, gFine, gCoarse, moistEff;
          R mK = 0;       // Opt: row 6, wave W's methane moisture term
          ringNew = 0.0;  // LDS ring: the value this step evicts, read in the same round trip
          double minNStep = 0.0;   // NCyc: wave S's mineral nitrogen at the start of this step
          int minNSeq = 0;
          {
            WAIT_BEGIN()
            if (NCyc)   // rows 0 1 3 4 and the plain soil Q10 factor (row 6, carried in `moistEff`'s place) + the mineral N
              takeFactorsN(&mailFac[t & 1][0][lane], &seqFac, &mailMinN[t & 1][lane], &seqMinN, t, g1, g2, gFine, gCoarse,
                           moistEff, minNStep, minNSeq);
            else if (Opt && RingLds)
              takeFactorsRing7(&mailFac[t & 1][0][lane], seqFacMoist, ldsAddr(&ringL[readSlot * 64 + lane]), t, g1,
                               g2, qSoilT, gFine, gCoarse, moistEff, mK, ringNew);
            else if (Opt)
              takeFactors7(&mailFac[t & 1][0][lane], seqFacMoist, t, g1, g2, qSoilT, gFine, gCoarse, moistEff, mK);
            else if (RingLds) {
              if constexpr (Carried)
                takeFactorsRing(ldsPtr<const R>(cFac), seqFacMoist, cRead, t, g1, g2, qSoilT, gFine, gCoarse, moistEff, ringNew);
              else
              takeFactorsRing(&mailFac[t & 1][0][lane], seqFacMoist, ldsAddr(&ringL[readSlot * 64 + lane]), t, g1,
                              g2, qSoilT, gFine, gCoarse, moistEff, ringNew);
            } else
              takeFactors(&mailFac[t & 1][0][lane], seqFacMoist, t, g1, g2, qSoilT, gFine, gCoarse, moistEff);
            WAIT_END(0)
          }
          // (Carried: each carried value is advanced once its last use of the step is behind it, in place -- the empty asm keeps
          // the compiler from deriving anything from the old value -- and WHERE among the step's three stretches of straight code
          // each one stands is what holds the loop heads at their measured offsets: tests/test_code_placement.py)
          // (Carried) lai(t + 1) FIRST: waves L and W start on step t + 1 with it, and by night their answer (the factors of
          // t + 1) and this wave's own step are nearly as long as each other -- left to the scheduler the post stood behind 36
          // instructions of the other pools' arithmetic.  The leaf pool's share of the step is computed HERE, once -- its litter,
          // its creation, the leaf part of checkNegativeCreation(), the pool of t + 1 -- then the post and a fence nothing is
          // moved across; the statements below take these values where the other instantiations compute them in place.
          [[maybe_unused]] R leafLitterFirst = 0, leafCreationFirst = 0, leafDeficitFirst = 0;
          [[maybe_unused]] double leafNextFirst = 0.0;
          if constexpr (Carried) {
            cRead += 512;
            asm volatile("" : "+v"(cRead));
            const R leafNow = (R)plantLeafC;
            leafLitterFirst = leafNow * K_ltr;
            leafCreationFirst = (R)(ringSum * 0.2) * K_la;
            leafDeficitFirst = rminv(ffma(leafNow, invLen, leafCreationFirst) - leafLitterFirst, R(0));
            leafNextFirst = plantLeafC;
            accum(leafNextFirst, (leafCreationFirst - leafDeficitFirst) - leafLitterFirst, len);
            post(ldsPtr<R>(cLai), &seqLai, (R)rmax0(leafNextFirst) * K_invLcsw, cSeq);
            __builtin_amdgcn_sched_barrier(0);
          }
          const R fSoil = NCyc ? R(0) : qSoilT * moistEff;
          rvN = 0;
          if (!RingLds) {
            if (sizeof(R) == 8)
              asm volatile("global_load_dwordx2 %0, %1, off" : "=&v"(rvN) : "v"(ringp + (uint32_t)readSlot * ncu) : "memory");
            else
              asm volatile("global_load_dword %0, %1, off" : "=&v"(rvN) : "v"(ringp + (uint32_t)readSlot * ncu) : "memory");
          }
          useLast = readSlot == lastIns;
          const bool isDay = Carried ? (dayMask & (1u << (t & 31))) != 0 : (dayMask & 1u) != 0;

          const R eLeaf = (R)plantLeafC, eSoilC = (R)soilC;
          const R eCoarse = (R)coarseRootC, eFine = (R)fineRootC;
          const R totalWoodC = (R)(plantWoodC + delta);
          const R meanNpp = (R)(ringSum * 0.2);
          const R folResp = eLeaf * g1;
          rVeg = ffma(totalWoodC, g2, folResp);
          if (Ext) rVeg += rmax0(X_growthFrac * meanNpp);   // vegResp2(), sipnet.c:1084-1103 (+0 with the flag off)
          rCoarseRoot = eCoarse * gCoarse;
          rFineRoot = eFine * gFine;
          if (!Opt) rSoil = eSoilC * fSoil;
          const R woodLitter = totalWoodC * K_wtr;
          const R leafLitter = Carried ? leafLitterFirst : eLeaf * K_ltr;
          R leafCreation = Carried ? leafCreationFirst : meanNpp * K_la, woodCreation = meanNpp * K_wa;
          const R coarseRootLoss = K_crt * eCoarse, fineRootLoss = K_frt * eFine;
          R coarseRootCreation = K_ca * meanNpp, fineRootCreation = K_fa * meanNpp;
          {  // checkNegativeCreation(), limitations.c:146-182, as selects
            const R leafDeficit = ffma(eLeaf, invLen, leafCreation) - leafLitter;
            const R ld = Carried ? leafDeficitFirst : rminv(leafDeficit, R(0));
            woodCreation += ld;
            leafCreation -= ld;
            const R fineDef = ffma(eFine, invLen, fineRootCreation) - fineRootLoss;
            const R coarseDef = ffma(eCoarse, invLen, coarseRootCreation) - coarseRootLoss;
            const bool fNeg = fineDef < R(0), cNeg = coarseDef < R(0);
            const R shift = (fNeg != cNeg) ? (fNeg ? fineDef : -coarseDef) : R(0);
            coarseRootCreation += shift;
            fineRootCreation -= shift;
          }
          if (NCyc)   // the plants' side of the step for wave S, and checkNitrogenLimitation() (see the general step)
            plantSideN(t, len, invLen, minNStep, minNSeq, (double)moistEff, (double)h0.x, leafLitter, woodLitter, fineRootLoss,
                       coarseRootLoss, R(0), R(0), leafCreation, woodCreation, fineRootCreation, coarseRootCreation);
          if constexpr (Carried) plantLeafC = leafNextFirst;   // (the pool of t + 1, as posted)
          else accum(plantLeafC, leafCreation - leafLitter, len);
          if constexpr (!Carried) post(&mailLai[(t + 1) & 1][lane], &seqLai, (R)rmax0(plantLeafC) * K_invLcsw, t + 1);   // (Carried: posted above)
          accum(plantWoodC, woodCreation - woodLitter, len);
          accum(coarseRootC, coarseRootCreation - coarseRootLoss, len);
          accum(fineRootC, fineRootCreation - fineRootLoss, len);
          if (Opt)
            optSoilSide(eSoilC, (R)litterC, eSoilC, fSoil, qSoilT, mK, coarseRootLoss + fineRootLoss, woodLitter + leafLitter, len,
                        rSoil, rHet, soilGain, litterGain, methaneReg);
          else if (!NCyc) soilGain = (double)((coarseRootLoss + fineRootLoss + woodLitter + leafLitter - rSoil) * len);
          const R r_a = rVeg + rFineRoot + rCoarseRoot;
          const R alloc = leafCreation + woodCreation + fineRootCreation + coarseRootCreation;
          // (Carried: the mortality test as lane masks straight from the compares -- one scalar test against the full wave)
          [[maybe_unused]] uint64_t okMask = 0;
          if constexpr (Carried)
            okMask = __builtin_amdgcn_ballot_w64(plantWoodC > kTiny) & __builtin_amdgcn_ballot_w64(fineRootC + coarseRootC > kTiny);
          else rootsOk = (plantWoodC > kTiny) && (fineRootC + coarseRootC > kTiny);
          photosynthesis = 0;
          if (__builtin_expect(isDay, 0)) {  // laid out for the night step: by night this wave is the critical one
            WAIT_BEGIN()
            if constexpr (Carried) COOP_CARRIED_PAD(2);   // (day steps only: the carbon wave has slack then)
            if constexpr (Carried) photosynthesis = take(ldsPtr<const R>(sumPsnLai - cLai), &seqPsn, t);
            else photosynthesis = take(&mailPsn[t & 1][lane], &seqPsn, t);
            WAIT_END(1)
          }
          accum(delta, (photosynthesis - r_a) - alloc, len);
          if constexpr (Carried) {
            okMask &= __builtin_amdgcn_ballot_w64(plantWoodC + delta > kTiny);
            if (__builtin_expect(okMask != allLanes, 0)) {
              dyingStep = true;
              break;
            }
          }
          const bool dies = !Carried && !(rootsOk && (plantWoodC + delta > kTiny));
          if (__builtin_expect(__builtin_amdgcn_ballot_w64(dies) != 0, 0)) {
            dyingStep = true;
            break;
          }
          finishStep(std::false_type{});
          if constexpr (Carried) {
            // (the 8-byte encoding: four bytes of padding in this stretch that no instruction slot pays for)
            asm volatile("v_sub_u32_e64 %0, %1, %0" : "+v"(cFac) : "v"(sumFac));
            cLai = sumLai - cLai;
            asm volatile("" : "+v"(cLai));
            if (__builtin_expect(t == wrapNext, 0)) {   // the next step uses slot 0
              if (t == wrapRead) cRead -= SIPNET_RING_SLOTS * 512;
              if (t == wrapIns) cIns -= SIPNET_RING_SLOTS * 512;
              wrapNext = wrapRead > wrapIns ? wrapRead : wrapIns;
            }
            cSeq++;
            cAlive = sumAlive - cAlive;
            cIns += 512;
            asm volatile("" : "+v"(cSeq), "+v"(cAlive), "+v"(cIns));
          } else {
          readSlot = nextSlot(readSlot);
          insSlot = nextSlot(insSlot);
          }
          MARK("C regular step end")
        }
        // (Carried: both ways out of the loop meet HERE, at an opaque copy of the flag: with one exit block the compiler keeps
        // fewer flag tests inside the loop than when it threads the dying exit into the divergent mortality code below)
        if constexpr (Carried) {
          int dying = uni((int)dyingStep);
          asm volatile("" : "+s"(dying));
          dyingStep = dying != 0;
        }
        if (dyingStep) {  // finish that step with the mortality code; the general step from the next one on
          if constexpr (Carried) rootsOk = (plantWoodC > kTiny) && (fineRootC + coarseRootC > kTiny);
          finishStep(std::true_type{});
          t++;
        }
        recB += (int)(t - tFirst) * (int)sizeof(FastRec);
        if constexpr (Carried) COOP_CARRIED_PAD(3);
      }
    }
  for (; t < tLast; t++, recB += sizeof(FastRec)) {
#pragma clang fp contract(off)  // explicit fused multiply-adds only: see the regular-tile path
    // record fields of the carbon block (len invLen | tsoil10 cumGdd | dayTime w0 | ints) and the
    // five factors of wave F / L and wave W's moisture effect for this step, in ONE LDS round trip; each flag is read before
    // the values (DS reads return in order), so a current flag vouches for what follows it
    d2 q0, q6, q7;
    i4 j0;
    R g1, g2, qSoilT, gFine, gCoarse, moistEff;
    R mK = 0;   // Opt: row 6 of the factor block, wave W's methane moisture term
    int facSeq, moistSeq;
    double minNStep = 0.0;   // NCyc: wave S's mineral nitrogen at the start of this step
    if (Opt) {
      // as the default take below, with row 6 (behind wave W's flag, like row 5)
      WAIT_BEGIN()
      const unsigned fac = ldsAddr(&mailFac[t & 1][0][lane]);
      const unsigned mst = ldsAddr(&mailFac[t & 1][5][lane]);
      WAIT_DO {
        if (sizeof(R) == 8) {
          asm volatile("ds_read_b128 %0, %13\n\tds_read_b128 %1, %13 offset:96\n\tds_read_b128 %2, %13 offset:112\n\t"
                       "ds_read_b128 %3, %13 offset:128\n\tds_read_b32 %4, %14\n\t"
                       "ds_read_b64 %5, %15\n\tds_read_b64 %6, %15 offset:512\n\tds_read_b64 %7, %15 offset:1024\n\t"
                       "ds_read_b64 %8, %15 offset:1536\n\tds_read_b64 %9, %15 offset:2048\n\t"
                       "ds_read_b32 %10, %16\n\tds_read_b64 %11, %17\n\tds_read_b64 %12, %17 offset:512\n\ts_waitcnt lgkmcnt(0)"
                       : "=&v"(q0), "=&v"(q6), "=&v"(q7), "=&v"(j0), "=&v"(facSeq), "=&v"(g1), "=&v"(g2),
                         "=&v"(qSoilT), "=&v"(gFine), "=&v"(gCoarse), "=&v"(moistSeq), "=&v"(moistEff), "=&v"(mK)
                       : "v"(ldsAddr(recB)), "v"(ldsAddr(&seqFac)), "v"(fac), "v"(ldsAddr(&seqMoist)), "v"(mst)
                       : "memory");
        } else {
          asm volatile("ds_read_b128 %0, %13\n\tds_read_b128 %1, %13 offset:96\n\tds_read_b128 %2, %13 offset:112\n\t"
                       "ds_read_b128 %3, %13 offset:128\n\tds_read_b32 %4, %14\n\t"
                       "ds_read_b32 %5, %15\n\tds_read_b32 %6, %15 offset:256\n\tds_read_b32 %7, %15 offset:512\n\t"
                       "ds_read_b32 %8, %15 offset:768\n\tds_read_b32 %9, %15 offset:1024\n\t"
                       "ds_read_b32 %10, %16\n\tds_read_b32 %11, %17\n\tds_read_b32 %12, %17 offset:256\n\ts_waitcnt lgkmcnt(0)"
                       : "=&v"(q0), "=&v"(q6), "=&v"(q7), "=&v"(j0), "=&v"(facSeq), "=&v"(g1), "=&v"(g2),
                         "=&v"(qSoilT), "=&v"(gFine), "=&v"(gCoarse), "=&v"(moistSeq), "=&v"(moistEff), "=&v"(mK)
                       : "v"(ldsAddr(recB)), "v"(ldsAddr(&seqFac)), "v"(fac), "v"(ldsAddr(&seqMoist)), "v"(mst)
                       : "memory");
        }
      } WAIT_WHILE(uni(facSeq) < t || uni(moistSeq) < t, 25, t);
      WAIT_END(0)
    } else if (NCyc) {
      // record fields, wave F's factors (rows 0 1 3 4 and the plain soil Q10 factor, row 6 -- carried in
      // `moistEff`'s place) and wave S's mineral nitrogen, each behind its flag, one round trip
      WAIT_BEGIN()
      const unsigned fac = ldsAddr(&mailFac[t & 1][0][lane]);
      const unsigned mnn = ldsAddr(&mailMinN[t & 1][lane]);
      WAIT_DO {
        if (sizeof(R) == 8) {
          asm volatile("ds_read_b128 %0, %12\n\tds_read_b128 %1, %12 offset:96\n\tds_read_b128 %2, %12 offset:112\n\t"
                       "ds_read_b128 %3, %12 offset:128\n\tds_read_b32 %4, %13\n\t"
                       "ds_read_b64 %5, %14\n\tds_read_b64 %6, %14 offset:512\n\tds_read_b64 %7, %14 offset:3072\n\t"
                       "ds_read_b64 %8, %14 offset:1536\n\tds_read_b64 %9, %14 offset:2048\n\t"
                       "ds_read_b32 %10, %15\n\tds_read_b64 %11, %16\n\ts_waitcnt lgkmcnt(0)"
                       : "=&v"(q0), "=&v"(q6), "=&v"(q7), "=&v"(j0), "=&v"(facSeq), "=&v"(g1), "=&v"(g2),
                         "=&v"(moistEff), "=&v"(gFine), "=&v"(gCoarse), "=&v"(moistSeq), "=&v"(minNStep)
                       : "v"(ldsAddr(recB)), "v"(ldsAddr(&seqFac)), "v"(fac), "v"(ldsAddr(&seqMinN)), "v"(mnn)
                       : "memory");
        } else {
          asm volatile("ds_read_b128 %0, %12\n\tds_read_b128 %1, %12 offset:96\n\tds_read_b128 %2, %12 offset:112\n\t"
                       "ds_read_b128 %3, %12 offset:128\n\tds_read_b32 %4, %13\n\t"
                       "ds_read_b32 %5, %14\n\tds_read_b32 %6, %14 offset:256\n\tds_read_b32 %7, %14 offset:1536\n\t"
                       "ds_read_b32 %8, %14 offset:768\n\tds_read_b32 %9, %14 offset:1024\n\t"
                       "ds_read_b32 %10, %15\n\tds_read_b64 %11, %16\n\ts_waitcnt lgkmcnt(0)"
                       : "=&v"(q0), "=&v"(q6), "=&v"(q7), "=&v"(j0), "=&v"(facSeq), "=&v"(g1), "=&v"(g2),
                         "=&v"(moistEff), "=&v"(gFine), "=&v"(gCoarse), "=&v"(moistSeq), "=&v"(minNStep)
                       : "v"(ldsAddr(recB)), "v"(ldsAddr(&seqFac)), "v"(fac), "v"(ldsAddr(&seqMinN)), "v"(mnn)
                       : "memory");
        }
      } WAIT_WHILE(uni(facSeq) < t, 26, t);   // (`moistSeq`: the mineral nitrogen's flag, looked at in plantSideN)
      qSoilT = 0;
      WAIT_END(0)
    } else {
      WAIT_BEGIN()
      const unsigned fac = ldsAddr(&mailFac[t & 1][0][lane]);
      const unsigned mst = ldsAddr(&mailFac[t & 1][5][lane]);
      // (re-reading the record while spinning is harmless; one asm statement defines every value,
      // so no copies are needed when the first look already finds the flags current)
      WAIT_DO {
        if (sizeof(R) == 8) {
          asm volatile("ds_read_b128 %0, %12\n\tds_read_b128 %1, %12 offset:96\n\tds_read_b128 %2, %12 offset:112\n\t"
                       "ds_read_b128 %3, %12 offset:128\n\tds_read_b32 %4, %13\n\t"
                       "ds_read_b64 %5, %14\n\tds_read_b64 %6, %14 offset:512\n\tds_read_b64 %7, %14 offset:1024\n\t"
                       "ds_read_b64 %8, %14 offset:1536\n\tds_read_b64 %9, %14 offset:2048\n\t"
                       "ds_read_b32 %10, %15\n\tds_read_b64 %11, %16\n\ts_waitcnt lgkmcnt(0)"
                       : "=&v"(q0), "=&v"(q6), "=&v"(q7), "=&v"(j0), "=&v"(facSeq), "=&v"(g1), "=&v"(g2),
                         "=&v"(qSoilT), "=&v"(gFine), "=&v"(gCoarse), "=&v"(moistSeq), "=&v"(moistEff)
                       : "v"(ldsAddr(recB)), "v"(ldsAddr(&seqFac)), "v"(fac), "v"(ldsAddr(&seqMoist)), "v"(mst)
                       : "memory");
        } else {
          asm volatile("ds_read_b128 %0, %12\n\tds_read_b128 %1, %12 offset:96\n\tds_read_b128 %2, %12 offset:112\n\t"
                       "ds_read_b128 %3, %12 offset:128\n\tds_read_b32 %4, %13\n\t"
                       "ds_read_b32 %5, %14\n\tds_read_b32 %6, %14 offset:256\n\tds_read_b32 %7, %14 offset:512\n\t"
                       "ds_read_b32 %8, %14 offset:768\n\tds_read_b32 %9, %14 offset:1024\n\t"
                       "ds_read_b32 %10, %15\n\tds_read_b32 %11, %16\n\ts_waitcnt lgkmcnt(0)"
                       : "=&v"(q0), "=&v"(q6), "=&v"(q7), "=&v"(j0), "=&v"(facSeq), "=&v"(g1), "=&v"(g2),
                         "=&v"(qSoilT), "=&v"(gFine), "=&v"(gCoarse), "=&v"(moistSeq), "=&v"(moistEff)
                       : "v"(ldsAddr(recB)), "v"(ldsAddr(&seqFac)), "v"(fac), "v"(ldsAddr(&seqMoist)), "v"(mst)
                       : "memory");
        }
      } WAIT_WHILE(uni(facSeq) < t || uni(moistSeq) < t, 27, t);
      WAIT_END(0)
    }
    if constexpr (Carried) COOP_CARRIED_PAD(4);
    const R fSoil = qSoilT * moistEff;
    const double* rare = (const double*)(recB + 144);
    const int32_t* rareI = (const int32_t*)(recB + 184);
    CSTAMP(0)
    const R len = (R)q0.x, invLen = (R)q0.y;
    const int bits = uni(j0.x);
    const int slots = uni(j0.y);
    const int insSlot = uni(j0.z);
    const int nEv = uni(j0.w);
    const int evSlot0 = slots & 255, evSlot1 = (slots >> 8) & 255;
    // HBM ring: the values this step evicts are requested now (asm: see the note on waits) and
    // awaited once, right before they are needed at the end of the step
    R rv0 = 0, rv1 = 0;
    if (!RingLds) {
      if (sizeof(R) == 8)
        asm volatile("global_load_dwordx2 %0, %2, off\n\tglobal_load_dwordx2 %1, %3, off"
                     : "=&v"(rv0), "=&v"(rv1)
                     : "v"(ringp + (uint32_t)evSlot0 * ncu), "v"(ringp + (uint32_t)evSlot1 * ncu) : "memory");
      else
        asm volatile("global_load_dword %0, %2, off\n\tglobal_load_dword %1, %3, off"
                     : "=&v"(rv0), "=&v"(rv1)
                     : "v"(ringp + (uint32_t)evSlot0 * ncu), "v"(ringp + (uint32_t)evSlot1 * ncu) : "memory");
    }
    const bool useLast0 = evSlot0 == lastIns, useLast1 = evSlot1 == lastIns;

    const bool alive0 = aliveC;
    const R eWood = (R)plantWoodC, eLeaf = (R)plantLeafC, eSoilC = (R)soilC;
    const R eCoarse = (R)coarseRootC, eFine = (R)fineRootC;
    const R eLitter = (R)litterC;   // (Opt) before this step's events, like every pool the fluxes look at
    const R totalWoodC = (R)(plantWoodC + delta);
    // getMassTotals() before the pool updates, balance.c:13-36 (carbon; default flags)
    double preC = 0.0;
    if (wantDiag) preC = (plantWoodC + delta) + plantLeafC + fineRootC + coarseRootC + soilC + (Opt && F_litterPool ? litterC : 0.0);
    R recLeafOffComputed = 0, recEvLeafOn = 0, recEvLeafOnFromWood = 0, recEvLeafOffLitter = 0;
    R evInC = 0, evOutC = 0;
    [[maybe_unused]] R evInN = 0, evOutN = 0;   // NCyc: the events' nitrogen input / output (events.c:530-541, :582-594, :660-672)
    // the plant side's share of getMassTotals() (balance.c:13-36): carbon, and nitrogen through the fixed C:N ratios
    auto plantMassC = [&]() -> double { return (plantWoodC + delta) + plantLeafC + fineRootC + coarseRootC; };
    auto plantMassN = [&]() -> double {
      return plantWoodC * (double)G_iWoodCN + plantLeafC * (double)G_iLeafCN + fineRootC * (double)G_iFineCN + coarseRootC * (double)G_iWoodCN;
    };
    double dgPreC = 0.0, dgPreN = 0.0, dgPostC = 0.0, dgPostN = 0.0;
    if (wantDiagN) {
      dgPreC = plantMassC();
      dgPreN = plantMassN();
    }

    auto leafOnNFromC = [&](R leafOnC) -> R {  // nitrogen.c:84-86
      return rmax0(leafOnC * G_iLeafCN - leafOnC * G_iWoodCN);
    };
    auto leafOnLimit = [&](R flux) -> R {  // limitations.c:13-64
      const R cDemand = flux * len;
      if (cDemand < R(kTiny)) return flux;
      R lim = fdiv((eWood + eCoarse) * PRM_RARE(leafOnReallocFrac), cDemand);
      if (NCyc) {  // the storage nitrogen is wave W's: its value at the start of this step
        double sN;
        takeD1(&mailStorN[t & 1][lane], &seqStorN, t, sN);
        const R nDemand = leafOnNFromC(cDemand);
        if (nDemand > R(kTiny)) lim = rminv(lim, fdiv((R)sN, nDemand));
      }
      lim = clip01(lim);
      return lim < R(1) ? flux * lim : flux;
    };

    const R meanNpp = (R)(ringSum * 0.2);

    // vegResp(), calcRootResp(), calcSoilRespiration() with wave W's factors
    const R folResp = eLeaf * g1;
    R rVeg = ffma(totalWoodC, g2, folResp);
    if (Ext) rVeg += rmax0(X_growthFrac * meanNpp);   // vegResp2(), sipnet.c:1084-1103 (+0 with the flag off)
    const R rCoarseRoot = eCoarse * gCoarse;
    const R rFineRoot = eFine * gFine;
    R rSoil = (NCyc || Opt) ? R(0) : eSoilC * fSoil;   // (Opt: optSoilSide, after the events)
    R rHet = 0;

    const R woodLitter = totalWoodC * K_wtr;
    R leafLitter = eLeaf * K_ltr;
    R leafCreation = meanNpp * K_la, woodCreation = meanNpp * K_wa;

    R leafOnCreation = 0, leafOnFromWood = 0;
    R evLeafOnAll = 0;   // NCyc: leaf-on by event (its nitrogen is part of the step's claim on the storage)
    const bool phenMay = (!allOn && q6.y >= minGddOn) || (!allOff && q7.x >= minOffDay);

    const R coarseRootLoss = K_crt * eCoarse, fineRootLoss = K_frt * eFine;
    R coarseRootCreation = K_ca * meanNpp, fineRootCreation = K_fa * meanNpp;

    // checkNegativeCreation(), limitations.c:146-182, as selects
    {
      const R leafDeficit = ffma(eLeaf, invLen, leafCreation) - eLeaf * K_ltr;
      const R ld = rminv(leafDeficit, R(0));
      woodCreation += ld;
      leafCreation -= ld;
      const R fineDef = ffma(eFine, invLen, fineRootCreation) - fineRootLoss;
      const R coarseDef = ffma(eCoarse, invLen, coarseRootCreation) - coarseRootLoss;
      const bool fNeg = fineDef < R(0), cNeg = coarseDef < R(0);
      const R shift = (fNeg != cNeg) ? (fNeg ? fineDef : -coarseDef) : R(0);
      coarseRootCreation += shift;
      fineRootCreation -= shift;
    }

    CSTAMP(1)

    // events (carbon side; irrigation belongs to wave W) and the yearly phenology switches
    if (__builtin_expect(nEv > 0 || (bits & FAST_PHEN_NEW_YEAR) ||
                         __builtin_amdgcn_ballot_w64(phenMay) != 0, 0)) {
      if (bits & FAST_PHEN_NEW_YEAR) phenBits = 0;
      const bool doOn = !(phenBits & 1) && q6.y >= gddLeafOn;
      const bool doOff = !(phenBits & 2) && q7.x >= leafOffDay;
      if (doOn) {
        const R leafOn = leafOnLimit(PRM_RARE(leafGrowth) * invLen);
        leafOnCreation = leafOn;
        const R src = eWood + eCoarse;
        if (src > R(kTiny)) leafOnFromWood = fdiv(leafOn * eWood, src);
        phenBits |= 1;
      }
      if (doOff) {
        const R off = (eLeaf * PRM_RARE(fracLeafFall)) * invLen;
        leafLitter += off;
        if (Full) recLeafOffComputed = off;
        phenBits |= 2;
      }
      allOn = __builtin_amdgcn_ballot_w64((phenBits & 1) == 0) == 0;
      allOff = __builtin_amdgcn_ballot_w64((phenBits & 2) == 0) == 0;
      R evLeafC = 0, evWoodC = 0, evFineRootC = 0, evCoarseRootC = 0;
      R evSoilC = 0, evLeafOnCreation = 0, evLeafOnFromWood = 0, evLeafOffLitter = 0;
      // NCyc: the soil side of the events (events.c:575-620, :660-672, :712-722, :778-789), for wave W
      R evLitterC = 0, evMinN = 0, evSoilOrgN = 0, evLitterN = 0, evLeafOffNResorp = 0;
      const bool toLitter = Opt && F_litterPool;   // Opt: above-ground transfers and organic carbon go to the litter pool
      const int ev0 = uni(rareI[3]);
      for (int k = 0; k < nEv; k++) {
        const EvRec& ev = a.events[evBase + ev0 + k];
        const int type = uni(ev.type);
        const R p0 = (R)ev.p[0], p1 = (R)ev.p[1], p2 = (R)ev.p[2], p3 = (R)ev.p[3];
        if (type == SIPNET_EV_PLANT) {
          evLeafC += p0 * invLen;
          evWoodC += p1 * invLen;
          evFineRootC += p2 * invLen;
          evCoarseRootC += p3 * invLen;
          if (Full) evInC += (p0 + p1 + p2 + p3) * invLen;  // events.c:530-541
          if (Full && NCyc) evInN += (p0 * G_iLeafCN + p1 * G_iWoodCN + p2 * G_iFineCN + p3 * G_iWoodCN) * invLen;
        } else if (type == SIPNET_EV_HARVEST) {
          const R woodC = totalWoodC;
          if (Full) evOutC += ((woodC + eLeaf) * p0 + (eFine + eCoarse) * p1) * invLen;  // events.c:582-594
          if (Full && NCyc)
            evOutN += ((eWood * G_iWoodCN + eLeaf * G_iLeafCN) * p0 + (eFine * G_iFineCN + eCoarse * G_iWoodCN) * p1) * invLen;
          if (NCyc) {
            evLitterC += (p2 * (eLeaf + woodC)) * invLen;
            evSoilC += (p3 * (eFine + eCoarse)) * invLen;
            evSoilOrgN += (p3 * (eFine * G_iFineCN + eCoarse * G_iWoodCN)) * invLen;
            evLitterN += (p2 * (eLeaf * G_iLeafCN + eWood * G_iWoodCN)) * invLen;
          } else if (toLitter) {   // events.c:575-580
            evLitterC += (p2 * (eLeaf + woodC)) * invLen;
            evSoilC += (p3 * (eFine + eCoarse)) * invLen;
          } else {
            evSoilC += (p3 * (eFine + eCoarse) + p2 * (eLeaf + woodC)) * invLen;
          }
          evLeafC += -eLeaf * (p0 + p2) * invLen;
          evWoodC += -woodC * (p0 + p2) * invLen;
          evFineRootC += -eFine * (p1 + p3) * invLen;
          evCoarseRootC += -eCoarse * (p1 + p3) * invLen;
        } else if (type == SIPNET_EV_FERT) {
          if (NCyc) {
            evLitterC += p1 * invLen;
            evLitterN += p0 * invLen;
            evMinN += p2 * invLen;
          } else if (toLitter) {
            evLitterC += p1 * invLen;
          } else {
            evSoilC += p1 * invLen;
          }
          if (Full) evInC += p1 * invLen;
          if (Full && NCyc) evInN += (p0 + p2) * invLen;
        } else if (type == SIPNET_EV_LEAFON) {
          const R flux = leafOnLimit(PRM_RARE(leafGrowth) * invLen);
          evLeafOnCreation += flux;
          const R src = eWood + eCoarse;
          if (src > R(kTiny)) evLeafOnFromWood += fdiv(flux * eWood, src);
        } else if (type == SIPNET_EV_LEAFOFF) {
          const R leafOff = eLeaf * PRM_RARE(fracLeafFall);
          evLeafOffLitter += leafOff * invLen;
          if (NCyc) {
            const R leafN = leafOff * G_iLeafCN;
            const R resorb = leafN * G_resorbC;
            evLeafOffNResorp += resorb * invLen;
            evLitterN += (leafN - resorb) * invLen;
          }
        }
      }
      if (NCyc) {
        evLeafOnAll = evLeafOnCreation;
        if (nEv > 0) {  // (W reads this block on every step whose record carries events)
          postD(&mailEvent[t & 1][0][lane], 0, (double)(evLitterC + evLeafOffLitter));
          postD(&mailEvent[t & 1][0][lane], 1, (double)evSoilC);
          postD(&mailEvent[t & 1][0][lane], 2, (double)evMinN);
          postD(&mailEvent[t & 1][0][lane], 3, (double)evSoilOrgN);
          postD(&mailEvent[t & 1][0][lane], 4, (double)evLitterN);
          postD(&mailEvent[t & 1][0][lane], 5, (double)(evLeafOffNResorp - leafOnNFromC(evLeafOnCreation)));
          postFlag(&seqEvent, t);
        }
      }
      if (Full) {
        recEvLeafOn = evLeafOnCreation;
        recEvLeafOnFromWood = evLeafOnFromWood;
        recEvLeafOffLitter = evLeafOffLitter;
      }
      plantWoodC += (double)(evWoodC * len);
      plantLeafC += (double)(evLeafC * len);
      if (!NCyc) soilC += (double)(evSoilC * len);
      plantWoodC -= (double)(evLeafOnFromWood * len);
      coarseRootC -= (double)((evLeafOnCreation - evLeafOnFromWood) * len);
      plantLeafC += (double)((evLeafOnCreation - evLeafOffLitter) * len);
      if (toLitter) {
        litterC += (double)(evLitterC * len);
        litterC += (double)(evLeafOffLitter * len);
      } else if (!NCyc) {
        soilC += (double)(evLeafOffLitter * len);
      }
      coarseRootC += (double)(evCoarseRootC * len);
      fineRootC += (double)(evFineRootC * len);
    }

    // ---- NCyc: the plants' side of the step for wave S, and checkNitrogenLimitation() (plantSideN)
    if (NCyc)
      plantSideN(t, len, invLen, minNStep, uni(moistSeq), (double)moistEff /* the plain soil Q10 factor */, q0.x, leafLitter, woodLitter,
                 fineRootLoss, coarseRootLoss, leafOnCreation, evLeafOnAll, leafCreation, woodCreation, fineRootCreation,
                 coarseRootCreation);

    CSTAMP(2)
    // the leaf pool of the next step does not involve this step's photosynthesis: update it
    // now and let wave L start on step t+1 (speculative only with respect to plant death)
    accum(plantLeafC, leafCreation + leafOnCreation - leafLitter, len);
    post(&mailLai[(t + 1) & 1][lane], &seqLai, (R)rmax0(plantLeafC) * K_invLcsw, t + 1);

    // plant pools that do not involve this step's photosynthesis (sipnet.c:1579-1626)
    accum(plantWoodC, woodCreation - woodLitter - leafOnFromWood, len);
    accum(coarseRootC, coarseRootCreation - coarseRootLoss - (leafOnCreation - leafOnFromWood), len);
    accum(fineRootC, fineRootCreation - fineRootLoss, len);
    double soilGain = 0.0, litterGain = 0.0;
    R methane = 0;
    if (Opt)
      optSoilSide(eSoilC, eLitter, (R)soilC, fSoil, qSoilT, mK, coarseRootLoss + fineRootLoss, woodLitter + leafLitter, len,
                  rSoil, rHet, soilGain, litterGain, methane);
    else if (!NCyc) soilGain = (double)((coarseRootLoss + fineRootLoss + woodLitter + leafLitter - rSoil) * len);
    const R r_a = rVeg + rFineRoot + rCoarseRoot;
    const R alloc = leafCreation + woodCreation + fineRootCreation + coarseRootCreation;
    const bool rootsOk = (plantWoodC > kTiny) && (fineRootC + coarseRootC > kTiny);

    // photosynthesis of this step (wave W after wave L); nights need no hand-over
    R photosynthesis = 0;
    if (bits & FAST_PAR_POS) {
      WAIT_BEGIN()
      photosynthesis = take(&mailPsn[t & 1][lane], &seqPsn, t);
      WAIT_END(1)
    }

    CSTAMP(3)
    // ---- pools (sipnet.c:1769-1806): plant pools first, so that the next step's leaf area
    // can leave for wave L as early as possible
    accum(delta, (photosynthesis - r_a) - alloc, len);
    double postC = 0.0;  // getMassTotals() after the pool updates (the soil pool's is still pending here)
    if (wantDiag)
      postC = (plantWoodC + delta) + plantLeafC + fineRootC + coarseRootC + (soilC + soilGain) +
              (Opt && F_litterPool ? litterC + litterGain : 0.0);
    if (wantDiagN) {
      dgPostC = plantMassC();
      dgPostN = plantMassN();
    }
    double deathWood = 0.0, deathRoot = 0.0;  // record columns 41, 42
    // checkForMortality(), sipnet.c:1688-1767
    bool alive = alive0;
    double deathToSoil0 = 0.0, deathToSoil1 = 0.0;
    bool diedNow = false;
    {
      const bool sufficient = rootsOk && (plantWoodC + delta > kTiny);
      // a ring epoch stays behind: the whole wavefront takes the general path from now on.  The flag
      // must stay wave-uniform -- set per lane it sent the survivors through the regular tiles and
      // the dead member through the general step of the same tile afterwards (found by the fuzzer:
      // a single member killed by a harvest, regular tiles following)
      if (__builtin_amdgcn_ballot_w64(sufficient != alive0) != 0) ringClean = false;
      if (__builtin_expect(sufficient != alive0, 0)) {
        if (!alive0) {
          alive = true;
        } else {
          alive = false;
          diedNow = true;
          if (diedAt < 0) diedAt = t;
          deathToSoil0 = fineRootC + coarseRootC;
          deathToSoil1 = plantWoodC + plantLeafC + delta;
          if (NCyc) {  // sipnet.c:1735-1746: to wave W's pools; posted before the verdict word that announces it
            postD(&mailDeath[0][lane], 0, deathToSoil0);
            postD(&mailDeath[0][lane], 1, deathToSoil1);
            postD(&mailDeath[0][lane], 2, fineRootC * (double)G_iFineCN + coarseRootC * (double)G_iWoodCN);
            postD(&mailDeath[0][lane], 3, plantWoodC * (double)G_iWoodCN + plantLeafC * (double)G_iLeafCN);
          }
          if (Full) {
            deathWood = plantWoodC + delta;
            deathRoot = deathToSoil0;
          }
          plantWoodC = 0.0;
          plantLeafC = 0.0;
          coarseRootC = 0.0;
          fineRootC = 0.0;
          delta = 0.0;
          ringSum = 0.0;
        }
      }
    }
    aliveC = alive;
    if (wantDiag || wantDiagN) {  // clamp warnings, sipnet.c:1346-1356
      clampWarn += (plantWoodC < 0.0 && fabs(plantWoodC) > kEps) + (plantLeafC < 0.0 && fabs(plantLeafC) > kEps) +
                   (coarseRootC < 0.0 && fabs(coarseRootC) > kEps) + (fineRootC < 0.0 && fabs(fineRootC) > kEps);
    }
    plantWoodC = rmax0(plantWoodC);
    plantLeafC = rmax0(plantLeafC);
    coarseRootC = rmax0(coarseRootC);
    fineRootC = rmax0(fineRootC);
    // NCyc: GPP - R_a of this step for wave S, which has R_h and forms NEE; before the verdict word
    if (NCyc) {
      postD(&mailPend[t & 1][0][lane], 0, (double)(photosynthesis * len - ffma(rVeg, len, (rCoarseRoot + rFineRoot) * len)));
      if (Full) {
        postD(&mailPend[t & 1][0][lane], 1, (double)ffma(rVeg, len, (rCoarseRoot + rFineRoot) * len));
        postD(&mailPend[t & 1][0][lane], 2, (double)((rCoarseRoot + rFineRoot) * len));
      }
      if constexpr (DiagOneSlot) {
      if (wantDiagN) {   // two chunks per workgroup: ONE slot of these rows -- S must be through with the step before's
        awaitAtLeast(&seqStorN, t);      // (S posts storN(t) right after its balance check of step t - 1; storN(tBegin) in its prologue)
        postD(&mailDiag[0][lane], 0, dgPreC);
        postD(&mailDiag[0][lane], 1, dgPreN);
        postD(&mailDiag[0][lane], 2, dgPostC);
        postD(&mailDiag[0][lane], 3, dgPostN);
        postD(&mailDiag[0][lane], 4, plantMassC());
        postD(&mailDiag[0][lane], 5, plantMassN());
        postD(&mailDiag[0][lane], 6, (double)photosynthesis + (double)evInC);
        postD(&mailDiag[0][lane], 7, (double)rVeg + (double)rFineRoot + (double)rCoarseRoot);
        postD(&mailDiag[0][lane], 8, (double)evOutC);
        postD(&mailDiag[0][lane], 9, (double)evInN);
        postD(&mailDiag[0][lane], 10, (double)evOutN);
      }
      }
      if (kPendRows > 3 && wantDiagN) {   // for wave S's balance check: totals before / after the updates / after the clamps, rates
        postD(&mailPend[t & 1][0][lane], 3, dgPreC);
        postD(&mailPend[t & 1][0][lane], 4, dgPreN);
        postD(&mailPend[t & 1][0][lane], 5, dgPostC);
        postD(&mailPend[t & 1][0][lane], 6, dgPostN);
        postD(&mailPend[t & 1][0][lane], 7, plantMassC());
        postD(&mailPend[t & 1][0][lane], 8, plantMassN());
        postD(&mailPend[t & 1][0][lane], 9, (double)photosynthesis + (double)evInC);
        postD(&mailPend[t & 1][0][lane], 10, (double)rVeg + (double)rFineRoot + (double)rCoarseRoot);
        postD(&mailPend[t & 1][0][lane], 11, (double)evOutC);
        postD(&mailPend[t & 1][0][lane], 12, (double)evInN);
        postD(&mailPend[t & 1][0][lane], 13, (double)evOutN);
      }
    }
    // confirms the lai(t+1) posted above, or revokes it when the stand died in this step (its
    // leaf pool was just zeroed); a stand that was never alive keeps its leaves and its lai
    postAlive(&mailAlive[(t + 1) & 1][lane], t + 1, diedNow);

    CSTAMP(4)
    soilC += soilGain;
    if (Opt) litterC += litterGain;
    if (!NCyc && __builtin_expect(__builtin_amdgcn_ballot_w64(diedNow) != 0, 0)) {
      if (diedNow) {
        soilC += deathToSoil0;
        if (Opt && F_litterPool) litterC += deathToSoil1;   // sipnet.c:1735-1746
        else soilC += deathToSoil1;
      }
    }
    if (wantDiag && soilC < 0.0 && fabs(soilC) > kEps) clampWarn++;
    soilC = rmax0(soilC);
    if (Opt && wantDiag && F_litterPool && litterC < 0.0 && fabs(litterC) > kEps) clampWarn++;
    if (Opt) litterC = rmax0(litterC);
    if (wantDiag) {  // updateBalanceTrackerPostClamp() + checkBalance(), balance.c:40-169
      const double finC = (plantWoodC + delta) + plantLeafC + fineRootC + coarseRootC + soilC + (Opt && F_litterPool ? litterC : 0.0);
      double clampedC = finC - postC;
      if (clampedC < kEps) clampedC = 0.0;
      double inC = ((double)photosynthesis + (double)evInC) * (double)len;
      const double outC = ((double)rVeg + (double)rFineRoot + (double)rCoarseRoot + (double)(Opt ? rHet : rSoil) +
                           (double)methane + (double)evOutC) * (double)len;
      inC += clampedC;
      const double dC = (finC - preC) - (inC - outC);
      maxDC = fmax(maxDC, fabs(dC));
      if (!(fabs(dC) < kEps)) balanceWarn++;
    }

    // ---- outputs: updateTrackers(), sipnet.c:1420-1496 ---------------------------------------
    const R tGpp = photosynthesis * len;
    const R tRh = (Opt ? rHet : rSoil) * len;
    const R tRa = ffma(rVeg, len, (rCoarseRoot + rFineRoot) * len);
    const R tNee = R(-1.0) * ((tGpp - tRa) - tRh);
    if (!NCyc) totNee += (double)tNee;
    R tRAbove = 0, tRRoot = 0, tRSoil = 0, tRtot = 0, tNpp = 0;
    if (Full) {
      if (bits & FAST_TRACK_NEW_YEAR) yGpp = yRtot = yRa = yRh = yNpp = yNee = 0.0;
      tRAbove = rVeg * len;
      tRRoot = (rCoarseRoot + rFineRoot) * len;
      tRSoil = tRRoot + tRh;
      tRtot = tRa + tRh;
      tNpp = tGpp - tRa;
      yGpp += (double)tGpp;
      yRa += (double)tRa;
      yRh += (double)tRh;
      yRtot += (double)tRtot;
      yNpp += (double)tNpp;
      yNee += (double)tNee;
      totRa += (double)tRa;
      totRh += (double)tRh;
      totRtot += (double)tRtot;
      totNpp += (double)tNpp;
      yLitter += (double)(leafLitter + recEvLeafOffLitter);
    }

    // ---- running mean of NPP (sipnet.c:1546-1570, runmean.c:61-116 via the plan) -------------
    const double npp = (double)(photosynthesis - rVeg - rCoarseRoot - rFineRoot);
    const double recMeanNpp = Full ? ringSum / 5.0 : 0.0;  // trackers.meanNPP: the mean BEFORE this step's insert
    CSTAMP(5)
    {
      if (!RingLds) asm volatile("s_waitcnt vmcnt(0)" : "+v"(rv0), "+v"(rv1) :: "memory");
      const double v0 = RingLds ? ringL[evSlot0 * 64 + lane] : (useLast0 ? lastNpp : (double)rv0);
      const int nOps = bits >> 16;
      // one or two evictions and a plain insert (two is the steady state of half-hourly forcing,
      // see the regular-tile path); with one eviction w1 is 0 and its term an exact no-op
      if (__builtin_expect(ringClean && insSlot >= 0 && nOps <= 2, 1)) {
        const double v1 = RingLds ? ringL[evSlot1 * 64 + lane] : (useLast1 ? lastNpp : (double)rv1);
        if constexpr (Carried) COOP_CARRIED_PAD(5);
        ringSum = ffma(-q7.y, v0, ringSum);
        ringSum = ffma(-rare[0], v1, ringSum);
        ringSum = ffma(npp, (double)len, ringSum);
      } else if (alive) {
        if (insSlot < 0) {
          ringSum = npp * 5.0;
        } else {
          double w0v = v0, w1v = RingLds ? ringL[evSlot1 * 64 + lane] : (useLast1 ? lastNpp : (double)rv1);
          if (ringValidFrom > 0) {
            if (uni(rareI[0]) < ringValidFrom) w0v = 0.0;
            if (uni(rareI[1]) < ringValidFrom) w1v = 0.0;
          }
          ringSum = ffma(-q7.y, w0v, ringSum);
          ringSum = ffma(-rare[0], w1v, ringSum);
          for (int k = 2; k < nOps; k++) {
            const RingOp& op = a.ringOps[opBase + uni(rareI[2]) + k];
            const int os = uni(op.slot);
            const double rvk = RingLds ? ringL[os * 64 + lane]
                                       : (os == lastIns ? lastNpp : (double)ringp[(uint32_t)os * ncu]);
            const double v = (uni(op.insStep) >= ringValidFrom) ? rvk : 0.0;
            ringSum = ffma(-op.w, v, ringSum);
          }
          ringSum = ffma(npp, (double)len, ringSum);
        }
      } else {
        ringValidFrom = t + 1;
      }
    }
    const int insEff = insSlot < 0 ? 0 : insSlot;
    if (RingLds) {
      ringL[insEff * 64 + lane] = npp;
    } else {
      ringp[(uint32_t)insEff * ncu] = (R)npp;
      lastIns = insEff;
      lastNpp = npp;
    }
    if (Full && recp) {  // the carbon / tracker columns of the strict kernel's record row
      double* __restrict__ r = recp;
      const int64_t L = a.ld;
      if (!NCyc) {   // (NCyc: wave S has the heterotrophic side and the soil / nitrogen pools, and writes these)
        r[0 * L] = (double)tNee;
        r[3 * L] = totNee;
        r[6 * L] = (double)tRSoil;
        r[9 * L] = (double)tRh;
        r[10 * L] = (double)tRtot;
        r[16 * L] = soilC;
        r[18 * L] = Opt ? litterC : cLitterC;
        r[22 * L] = cMinN;
        r[23 * L] = cSoilOrgN;
        r[24 * L] = cLitterN;
        r[25 * L] = cStorN;
        r[27 * L] = 0.0;
        r[28 * L] = 0.0;
        r[29 * L] = 0.0;
        r[30 * L] = 0.0;
        r[31 * L] = (double)(methane * len);
      }
      r[4 * L] = (double)tNpp;
      r[5 * L] = (double)tRAbove;
      r[7 * L] = (double)tRRoot;
      r[8 * L] = (double)tRa;
      r[11 * L] = (double)(woodCreation * len);
      r[14 * L] = plantWoodC;
      r[15 * L] = plantLeafC;
      r[20 * L] = coarseRootC;
      r[21 * L] = fineRootC;
      r[26 * L] = delta;
      r[32 * L] = recMeanNpp;
      r[33 * L] = rare[3];  // gddAfter
      r[34 * L] = rare[4];  // tillAfter
      r[36 * L] = (double)(leafOnCreation * len);
      r[37 * L] = (double)(leafOnFromWood * len);
      r[38 * L] = (double)(recLeafOffComputed * len);
      r[39 * L] = (double)(recEvLeafOn * len);
      r[40 * L] = (double)(recEvLeafOnFromWood * len);
      r[41 * L] = deathWood;
      r[42 * L] = deathRoot;
      r[43 * L] = diedNow ? 1.0 : 0.0;
      recp += (int64_t)SIPNET_NREC * L;
    }
    if constexpr (Sums && !NCyc) {
      sumsC.nee += (double)tNee;
      if (--sumsC.left == 0) {
        *oNee = (OutT)sumsC.nee;
        oNee += ldNee;
        sumsC.nee = 0.0;
        sumsC.left = a.sumEvery;
      }
    } else {
    if (!NCyc) {
      *oNee = tNee;
      oNee += ldNee;
    }
    }
    if (__builtin_expect(stageOn, 0)) postRaw(&stage[0][(t - tBegin) & (2 * kStageR - 1)][lane], tNee);
    CSTAMP(6)
  }  // steps of this tile
  }  // tiles
  if constexpr (Sums && !NCyc) {
    if (sumsC.left != a.sumEvery) *oNee = (OutT)sumsC.nee;   // the launch's last, shorter group
  }

  CSTAMP_STORE()
  WAIT_STORE(8)
  if constexpr (Carried) COOP_CARRIED_PAD(6);
  if (a.statsPart) {  // every NEE store of the launch has reached L2 (see wave L's statistics)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("ds_write_b32 %0, %1" :: "v"(ldsAddr(&seqDone[0])), "v"(1) : "memory");
  }
  if (act) {
    if (RingLds)
      for (int k = 0; k < SIPNET_RING_SLOTS; k++) ringp[(uint32_t)k * ncu] = (R)ringL[k * 64 + lane];
    ST(plantWoodC) = plantWoodC;
    ST(plantLeafC) = plantLeafC;
    if (!NCyc) ST(soilC) = soilC;
    if (Opt) ST(litterC) = litterC;
    ST(coarseRootC) = coarseRootC;
    ST(fineRootC) = fineRootC;
    ST(plantCAccountingDelta) = delta;
    ST(ringSum) = ringSum;
    if (!NCyc) ST(totNee) = totNee;
    ST(phenBits) = (double)phenBits;
    ST(ringValidFrom) = (double)ringValidFrom;
    ST(diedAt) = (double)diedAt;
    if (Full) {
      ST(totRa) = totRa;
      ST(totNpp) = totNpp;
      ST(yearlyGpp) = yGpp;
      ST(yearlyRa) = yRa;
      ST(yearlyNpp) = yNpp;
      ST(yearlyLitter) = yLitter;
      if (!NCyc) {   // (NCyc: the accumulators with R_h in them are wave S's)
        ST(totRtot) = totRtot;
        ST(totRh) = totRh;
        ST(yearlyRtot) = yRtot;
        ST(yearlyRh) = yRh;
        ST(yearlyNee) = yNee;
      }
    }
    if (wantDiag) {
      double* __restrict__ dg = a.diag + col;
      if (clampWarn) atomicAdd(dg, (double)clampWarn);  // the water wave adds its two pools' count
      dg[1 * nc] += (double)balanceWarn;
      dg[2 * nc] = fmax(dg[2 * nc], maxDC);
    }
    if (wantDiagN && clampWarn) atomicAdd(a.diag + col, (double)clampWarn);   // (the balance counters are wave S's)
  }
