// The exports of the host simulation that answer for launch_plan.hpp, inside an extern "C" block: part of sim.cpp (the whole
// host build) and all of launch_plan_sim.cpp (the plan alone, for tests that ask it next to a GPU run).
// The batch launchers' plan (launch_plan.hpp).  tune: the seven keys the rules read, in the order of
// tests/golden/launch_plan_parent.json's in_fields (-1 = no override); out: its out_fields.
static Tuning plan_tuning(const int64_t* tune) {
  static const int keys[7] = {D377_TUNE_SMALL_MAX, D377_TUNE_TINY_MAX, D377_TUNE_DECOMPRESS_CHUNKED_MIN, D377_TUNE_FB_WIDE, D377_TUNE_FB_K,
                              D377_TUNE_AFFINE_BLOCKS_PER_CU, D377_TUNE_CHUNK_PER_LANE};
  Tuning t;
  for (int k = 0; k < 7; ++k) t.v[keys[k]] = tune[k];
  return t;
}
static void plan_out(const LaunchPlan& p, int64_t codec_min, int64_t* out) {
  const int64_t v[10] = {p.route, p.grid, p.block, p.guard, codec_min, p.deal.nslots, p.deal.per_lane, p.deal.extra, p.deal.prio, p.deal.kmax};
  for (int i = 0; i < 10; ++i) out[i] = v[i];
}
// in = {op, aux, n, cus, tune[7]}
void sim_launch_plan(const int64_t* in, int64_t* out) {
  const Tuning t = plan_tuning(in + 4);
  PlanDev d; d.cus = (int)in[3]; d.tune = &t;
  const Op op = (Op)in[0];
  const bool codec = op == OP_DECOMPRESS || op == OP_COMPRESS || op == OP_ROUNDTRIP;
  plan_out(launch_plan(op, (int)in[1], (size_t)in[2], d), codec ? (int64_t)codec_chunked_min(d) : 0, out);
}
// The sums' route by their np sums or partial sums: a wave each up to sums_wave_max, else the lane deal that reads no tuning
// key (batch_host.hpp lane_chunks).  in = {np, cus, kmax, tiny_max}
void sim_sums_route(const int64_t* in, int64_t* out) {
  Tuning t;
  t.v[D377_TUNE_TINY_MAX] = in[3];
  PlanDev d; d.cus = (int)in[1]; d.tune = &t;
  const size_t np = (size_t)in[0];
  LaunchPlan p = plain_plan(ROUTE_WAVE_PER_ELEMENT, (int)np, 64);
  if (np > sums_wave_max(d)) {
    p = dealt_plan(ROUTE_LANE_SETS, lane_deal(d, np, PLAN_WAVES_PER_SIMD, (int)in[2], false));
    p.guard = false;                                           // (when a sum holds the guard is its unit's affair)
  }
  plan_out(p, 0, out);
}
// lane_deal in the generic launcher's form (tunable, chunk_per_lane = D377_TUNE_CHUNK_PER_LANE or -1).  out = {grid, nslots,
// per_lane, extra, prio, kmax}; consts = {BLOCK, WAVES_PER_SIMD, DCB_K, DCB_KMAX, DCB_K_LONG, FB_SETS, FB_K, PIPE_CHUNK}
void sim_lane_deal(int64_t count, int cus, int sets, int kmax, int64_t chunk_per_lane, int64_t* out, int64_t* consts) {
  Tuning t;
  t.v[D377_TUNE_CHUNK_PER_LANE] = chunk_per_lane;
  PlanDev d; d.cus = cus; d.tune = &t;
  const LaneDeal c = lane_deal(d, (size_t)count, sets, kmax, true);
  const int64_t v[6] = {c.grid, c.nslots, c.per_lane, c.extra, c.prio, c.kmax};
  for (int i = 0; i < 6; ++i) out[i] = v[i];
  const int64_t cs[8] = {PLAN_BLOCK, PLAN_WAVES_PER_SIMD, PLAN_DCB_K, PLAN_DCB_KMAX, PLAN_DCB_K_LONG, PLAN_FB_SETS, PLAN_FB_K, (int64_t)PIPE_CHUNK};
  for (int i = 0; i < 8; ++i) consts[i] = cs[i];
}
