// spark.cpp -- host orchestration of the SPARK half of vPIN's Spartan SNARK on one MI355X:
// the computation commitment and the sparse-polynomial evaluation proof that follow the sat proof
// on the same transcript.
//
// C++ counterpart of (names mirror the reference):
//   Spartan/src/lib.rs:294-359                    SNARKGens::new, SNARK::encode
//   Spartan/src/r1csinstance.rs:29-49,309-372     R1CSCommitmentGens, R1CSInstance::commit, R1CSEvalProof
//   Spartan/src/sparse_mlpoly.rs:42-1572          Derefs, AddrTimestamps, multi_commit, Layers,
//                                                 ProductLayerProof, HashLayerProof, PolyEvalNetworkProof,
//                                                 SparseMatPolyEvalProof
//   Spartan/src/product_tree.rs:258-385           ProductCircuitEvalProofBatched::prove
//   Spartan/src/sumcheck.rs:248-425               SumcheckInstanceProof::prove_cubic_batched
//   vPIN_proof_generation/src/commit_test.rs:59-133  my_lib_prove (whole)
// The gathers, the hash layer, the product trees, every sum-check round, the slice evaluations and the
// commitments run in spark.hip / msm.hip / poly.hip; this file owns the transcript, the per-round
// scalars and the bincode image.  It shares no code with the test-side checker.
#include <cstdio>

#include "host/proof_sizes.h"
#include "host/prover_common.h"
#include "gadget_dev.h"
#include "sc_dev.h"
#include "spark_dev.h"

namespace {

using namespace vpin_host;
using namespace vpin_prover;

// VPIN_SPARK_TRACE=1: finer spans of one proof on stderr (development aid)
static bool spark_trace() { static const bool on = getenv("VPIN_SPARK_TRACE") != nullptr; return on; }
struct TraceSpan {
  const char* name; Clock::time_point t0;
  explicit TraceSpan(const char* n) : name(n), t0(Clock::now()) {}
  ~TraceSpan() { if (spark_trace()) fprintf(stderr, "[spark] %-28s %8.3f ms\n", name, secs(t0, Clock::now()) * 1e3); }
};

// ---- generators: one stream under b"gens_r1cs_eval", three PolyCommitmentGens views -----------

struct SparkGens {
  std::vector<Point> g;                              // host copy of the stream prefix derived so far
  std::map<size_t, std::unique_ptr<PcGens>> views;  // by num_vars of the committed polynomial
};

static void spark_cache_free(vpin_ctx* c) {
  auto* sg = static_cast<SparkGens*>(c->spark_cache);
  if (!sg) return;
  delete sg;  // the device tables belong to the shared registry
  c->spark_cache = nullptr;
}

// table budget for the b"gens_r1cs_eval" stream: its largest user (the derefs commitment, 6N full-width
// scalars per proof) is the single most expensive step of a SNARK, and every window bit saves ~8 % of
// it, so on a 288 GB part the table gets up to 80 GB (11-bit windows for 32 770 generators)
static size_t spark_budget_gb(vpin_ctx* c) {
  // a process that proves once and exits sizes its tables by use, far below either budget (msm.hip gens_build), and the
  // first hipMemGetInfo of a process costs 35-50 ms: not asked then (a failed allocation still halves the table)
  if (c->expected_proofs > 0) return (size_t)24;
  static const size_t gb = [c] {
    const char* e = getenv("VPIN_SPARK_GENS_BUDGET_GB");
    if (e && atoi(e) > 0) return (size_t)atoi(e);
    // from the memory that is FREE when the first table of the stream is built (another tenant's allocations, a smaller
    // part); msm.hip's gens_build additionally caps every table at a third of the free memory of its moment
    size_t free_b = 0, total_b = 0;
    (void)hipSetDevice(c->device);
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return (size_t)24;
    return free_b >= ((size_t)200 << 30) ? (size_t)80 : (size_t)24;
  }();
  return gb;
}

// PolyCommitmentGens::new(ell, b"gens_r1cs_eval") (dense_mlpoly.rs:26-33; lib.rs:315-321)
static int get_view(vpin_ctx* c, size_t ell, const PcGens** out) {
  if (!c->spark_cache) { c->spark_cache = new SparkGens(); c->spark_cache_free = spark_cache_free; }
  auto* sg = static_cast<SparkGens*>(c->spark_cache);
  auto it = sg->views.find(ell);
  if (it == sg->views.end()) {
    const size_t left = ell / 2, R = (size_t)1 << (ell - left), nb = R + 2;
    // every MultiCommitGens::new(n, label) is a prefix of the same SHAKE stream
    vpin::TraceLap lap(nullptr, "spark get_view");
    if (sg->g.size() < nb) derive_gens(sg->g, nb, "gens_r1cs_eval", c);
    lap("derive_gens (host)");
    std::unique_ptr<PcGens> v(new PcGens());
    v->ell = ell; v->L = (size_t)1 << left; v->R = R;
    int rc = vpin::gens_shared_rows(c, "gens_r1cs_eval", nullptr, nb, 0, &v->dev);
    if (rc == VPIN_EINVAL) {
      std::vector<uint8_t> xyzt(128 * nb);
#pragma omp parallel for schedule(static) num_threads(host_threads())
      for (long i = 0; i < (long)nb; i++) sg->g[i].to_xyzt(xyzt.data() + 128 * (size_t)i);
      // full-size scalars one proof commits under this table: the derefs polynomial's six non-zero slices, 6N of the 16N
      // entries of the largest view (the computation commitment's entries are addresses, counters and small constants)
      c->gens_scalars_per_proof = (double)((size_t)1 << ell) * 0.375;
      rc = vpin::gens_shared_rows(c, "gens_r1cs_eval", xyzt.data(), nb, spark_budget_gb(c), &v->dev);
    }
    if (rc) return rc;
    lap("device table");
#pragma omp parallel for schedule(static, 1) num_threads(2)
    for (int k = 0; k < 2; k++) {
      if (k == 0) v->fb_gR = FixedBase(sg->g[R]);
      else v->fb_h = FixedBase(sg->g[R + 1]);
    }
    lap("fixed bases (host)");
    v->bind_views();
    it = sg->views.emplace(ell, std::move(v)).first;
  }
  *out = it->second.get();
  return VPIN_OK;
}

using Shape = vpin_sizes::SparkShape;  // host/proof_sizes.h: the sizes are plain arithmetic, shared with the proof record's codec

static Shape shape_of(size_t num_cons, size_t num_vars, const size_t nnz[3]) { return vpin_sizes::spark_shape(num_cons, num_vars, nnz); }

// DensePolynomial::commit(gens, None) (dense_mlpoly.rs:193-218): zero blinds
// short_scalars: most of Z is addresses, timestamps and counters (see vpin::hyrax_commit_walk)
static int commit_noblind(vpin_ctx* c, const PcGens* pc, const vpin_table* Z, std::vector<CG>& out, bool short_scalars = false) {
  std::vector<uint8_t> zeros(pc->L * 32, 0);
  out.resize(pc->L);
  if (short_scalars) return vpin::hyrax_commit_walk(c, pc->dev, Z, zeros.data(), pc->L, pc->R + 1, out[0].b);
  return vpin_hyrax_commit(c, pc->dev, Z, zeros.data(), pc->L, pc->R + 1, out[0].b);
}

static void append_polycomm(Transcript& tr, const char* label, const std::vector<CG>& C) {
  // PolyCommitment::append_to_transcript (dense_mlpoly.rs:305-313)
  tr.append_message(label, "poly_commitment_begin");
  for (auto& p : C) tr.append_point("poly_commitment_share", p.b);
  tr.append_message(label, "poly_commitment_end");
}

static void w_scalars(Writer& w, const Fq* v, size_t n) { w.u64(n); for (size_t i = 0; i < n; i++) w.scalar(v[i]); }

// PolyEvalProof::prove with blinds None, blind_Zr None (dense_mlpoly.rs:326-379)
// z_rows (one proof over several GPUs, split by residue class): this rank's rows rank, rank + world, .. of Z stored densely; Z then
// only gives the shape
// lz_pre / rv_pre (single GPU, SlicePass below): LZ = L^T Z and R = eq(r[left..], .) already known from the pass that evaluated
// the slices -- the table is not read again
static int polyeval_prove_plain(vpin_ctx* c, const PcGens& pc, const vpin_table* Z, const std::vector<Fq>& r, const Fq& Zr,
                                Transcript& tr, Transcript& tape, DpLog& out, const vpin::fq* z_rows = nullptr,
                                const std::vector<Fq>* lz_pre = nullptr, const std::vector<Fq>* rv_pre = nullptr) {
  if (r.size() != pc.ell || (!(lz_pre && rv_pre) && (!Z || Z->len != ((size_t)1 << pc.ell)))) return VPIN_ESHAPE;
  tr.append_protocol_name("polynomial evaluation proof");
  const size_t left = pc.ell / 2, right = pc.ell - left;
  if (lz_pre && rv_pre) {  // (Z may be null: the table is not needed)
    if (lz_pre->size() != pc.R || rv_pre->size() != pc.R) return VPIN_ESHAPE;
    TraceSpan ts("  dplog");
    return dplog_prove(c, pc, tr, tape, *lz_pre, Fq::zero(), *rv_pre, Zr, Fq::zero(), out);
  }
  std::vector<Fq> Lv(pc.L), Rv(pc.R), LZ(pc.R);
  host_eq(r.data(), left, Lv.data());
  host_eq(r.data() + left, right, Rv.data());
  int rc;
  {
    TraceSpan ts("  poly_bound");
    // one proof over several GPUs: every rank sums its block of rows, the partial vectors are all-gathered on the device
    if (c->comm && c->comm->world > 1) rc = vpin::poly_bound_dist(c, Z, B(Lv.data()), pc.L, B(LZ.data()), z_rows);
    else rc = vpin_poly_bound(c, Z, B(Lv.data()), pc.L, B(LZ.data()));
  }
  if (rc) return rc;
  if ((rc = vpin::comm_mark(c, "hash_poly_bound"))) return rc;
  TraceSpan ts("  dplog");
  return dplog_prove(c, pc, tr, tape, LZ, Fq::zero(), Rv, Zr, Fq::zero(), out);
}

// Single GPU: the slice evaluations of a combined polynomial and, later, the LZ vector of its evaluation proof from ONE pass
// over the table (poly.hip slices_bound / slices_combine).  nbits = log2 of the slice count, used = slices that are not
// identically zero, rand = the point the slices are evaluated at (log2 of the slice length challenges).
struct SlicePass {
  vpin::DevBuf lzs;
  std::vector<Fq> Rv;
  int used = 0, nbits = 0;
  bool on = false;
  explicit SlicePass(vpin_ctx* c) : lzs(c) {}
  static bool fits(const PcGens& pc, int nbits, const std::vector<Fq>& rand) {
    const bool off = getenv("VPIN_HASH_TWO_PASS") != nullptr;  // A/B and tests: the separate evaluation and bound passes (read per proof)
    return !off && pc.ell / 2 >= (size_t)nbits && rand.size() + (size_t)nbits == pc.ell;
  }
  // table32 / n32: the first n32 slices as u32 (the decommitment's addresses and timestamps); table: the other used - n32
  int run(vpin_ctx* c, const PcGens& pc, const uint32_t* table32, int n32, const vpin::fq* table, int nbits_, int used_,
          const std::vector<Fq>& rand, Fq* ev) {
    nbits = nbits_; used = used_;
    const size_t left = pc.ell / 2, T = pc.L >> nbits, N = (size_t)1 << rand.size();
    std::vector<Fq> Ltop(T);
    host_eq(rand.data(), left - (size_t)nbits, Ltop.data());
    Rv.resize(pc.R);
    host_eq(rand.data() + (left - (size_t)nbits), pc.ell - left, Rv.data());
    if (lzs.alloc((size_t)used * pc.R * 32)) return VPIN_ENOMEM;
    int rc = vpin::slices_bound(c, table32, n32, table, N, used, pc.R, B(Ltop.data()), T, B(Rv.data()), (vpin::fq*)lzs.p, B(ev));
    on = rc == VPIN_OK;
    return rc;
  }
  // LZ of the combined polynomial at (ch, rand): sum_s eq(ch, s) LZ_s
  int combine(vpin_ctx* c, const PcGens& pc, const std::vector<Fq>& ch, std::vector<Fq>& LZ) {
    std::vector<Fq> coef((size_t)1 << nbits);
    host_eq(ch.data(), (size_t)nbits, coef.data());
    LZ.resize(pc.R);
    return vpin::slices_combine(c, (const vpin::fq*)lzs.p, used, pc.R, B(coef.data()), B(LZ.data()));
  }
};

// ---- one proof over several GPUs: who owns which circuit, and the per-round exchange -------------------------------
// The 12 "ops" circuits and the 6 dot-product halves are proven in the same rounds, so they are dealt together (longest
// processing time first; an ops circuit folds 2 tables over all layers = 4 units, a dot-product half 3 tables on layer 0 = 3
// units); the 4 "mem" circuits form their own phase and go to the ranks with the least ops work.  Every rank computes
// the same plan.  Ranks own whole circuits: leaves, tree, every round and the persistent tails of a circuit stay on one
// GPU, and per round only its three scalars leave it.
struct DistPlan {
  vpin_comm* cm = nullptr;
  int rank = 0, world = 1;
  int owner_ops[12], owner_dotp[6], owner_mem[4];
  std::vector<std::vector<int>> ops_of, dotp_of, mem_of;  // per rank, ascending
  int max_ops_inst = 0, max_mem_inst = 0;                 // most instances (circuits + halves) any rank owns per phase
  int lw = 0;                                             // log2(world) when the proof is split by residue class, else 0
};

static void make_plan(int world, int owner_ops[12], int owner_dotp[6], int owner_mem[4]) {
  std::vector<long> load(world, 0);
  auto least = [&](const std::vector<long>& key2) {
    int best = 0;
    for (int r = 1; r < world; r++)
      if (load[r] < load[best] || (load[r] == load[best] && key2[r] < key2[best])) best = r;
    return best;
  };
  const std::vector<long> none(world, 0);
  for (int t = 0; t < 12; t++) { int r = least(none); owner_ops[t] = r; load[r] += 4; }
  for (int k = 0; k < 6; k++) { int r = least(none); owner_dotp[k] = r; load[r] += 3; }
  std::vector<long> ops_load = load;
  std::fill(load.begin(), load.end(), 0);
  for (int t = 0; t < 4; t++) { int r = least(ops_load); owner_mem[t] = r; load[r] += 1; }
}

static void plan_init(DistPlan& pl, vpin_comm* cm) {
  pl.cm = cm; pl.rank = cm->rank; pl.world = cm->world;
  make_plan(pl.world, pl.owner_ops, pl.owner_dotp, pl.owner_mem);
  pl.ops_of.assign(pl.world, {}); pl.dotp_of.assign(pl.world, {}); pl.mem_of.assign(pl.world, {});
  for (int t = 0; t < 12; t++) pl.ops_of[pl.owner_ops[t]].push_back(t);
  for (int k = 0; k < 6; k++) pl.dotp_of[pl.owner_dotp[k]].push_back(k);
  for (int t = 0; t < 4; t++) pl.mem_of[pl.owner_mem[t]].push_back(t);
  for (int r = 0; r < pl.world; r++) {
    pl.max_ops_inst = std::max(pl.max_ops_inst, (int)(pl.ops_of[r].size() + pl.dotp_of[r].size()));
    pl.max_mem_inst = std::max(pl.max_mem_inst, (int)pl.mem_of[r].size());
  }
}

// `per` scalars of each of this rank's instances (its circuits in ascending order, then -- with_dotp -- its dot-product
// halves) -> the same for ALL instances in the single-GPU slot order: circuit g at global[per*g], half k at global[per*(12+k)]
static int dist_exchange(vpin_ctx* c, const DistPlan& pl, bool mem, bool with_dotp, const Fq* local, int per, Fq* global,
                         const char* tag = nullptr) {
  const int maxi = mem ? pl.max_mem_inst : pl.max_ops_inst;
  const size_t chunk = (size_t)maxi * per;
  std::vector<Fq> sb(chunk, Fq::zero()), rb(chunk * pl.world);
  const auto& mine = mem ? pl.mem_of[pl.rank] : pl.ops_of[pl.rank];
  const size_t nloc = mine.size() + (with_dotp ? pl.dotp_of[pl.rank].size() : 0);
  if (nloc) memcpy(sb.data(), local, nloc * per * 32);
  int rc = vpin::comm_allgather_ctx(c, sb.data(), rb.data(), chunk * 32, tag);
  if (rc) return rc;
  for (int r = 0; r < pl.world; r++) {
    const Fq* src = rb.data() + (size_t)r * chunk;
    for (int g : (mem ? pl.mem_of[r] : pl.ops_of[r])) { memcpy(global + (size_t)per * g, src, (size_t)per * 32); src += per; }
    if (with_dotp)
      for (int k : pl.dotp_of[r]) { memcpy(global + (size_t)per * (12 + k), src, (size_t)per * 32); src += per; }
  }
  return VPIN_OK;
}

// ---- ProductCircuitEvalProofBatched::prove (product_tree.rs:258-385) ------------------------------

struct Batched {
  std::vector<std::vector<Fq>> polys, claims_left, claims_right;  // per layer, top layer first
  std::vector<Fq> dotp[3];
};

static void write_batched(Writer& w, const Batched& b) {
  w.u64(b.polys.size());
  for (size_t l = 0; l < b.polys.size(); l++) {
    w.u64(b.polys[l].size() / 3);  // SumcheckInstanceProof.compressed_polys
    for (size_t j = 0; j < b.polys[l].size() / 3; j++) w_scalars(w, &b.polys[l][3 * j], 3);
    w_scalars(w, b.claims_left[l].data(), b.claims_left[l].size());
    w_scalars(w, b.claims_right[l].data(), b.claims_right[l].size());
  }
  for (int k = 0; k < 3; k++) w_scalars(w, b.dotp[k].data(), b.dotp[k].size());
}

// The six DotProductCircuit halves ride along on layer 0 of the ops forest.  N leaves per half pair on this rank, vals = the
// three val slices (3 x N), derefs = the six derefs slices (6 x N): the whole tables, or -- split by residue class -- the
// rank's local entries.
struct DotpCtx {
  const vpin_spark_decomm* d;  // spark_collect reads the source tables through it (one GPU, launch-only end of a layer)
  size_t N;
  const vpin::fq* vals;
  const vpin::fq* derefs;
  vpin::fq* scratch;           // 18 x N / 4
  Fq claims[6];                // their evaluations (claim_eval_dotp_left/right per matrix)
};

// sum over ranks of `cnt` scalars per rank
static int dist_sum(vpin_ctx* c, const DistPlan& pl, const Fq* mine, size_t cnt, Fq* out, const char* tag) {
  std::vector<Fq> all(cnt * (size_t)pl.world);
  int rc = vpin::comm_allgather_ctx(c, mine, all.data(), cnt * 32, tag);
  if (rc) return rc;
  for (size_t i = 0; i < cnt; i++) {
    Fq a = Fq::zero();
    for (int r = 0; r < pl.world; r++) a = a + all[(size_t)r * cnt + i];
    out[i] = a;
  }
  return VPIN_OK;
}

// Split by residue class: the last cnt entries of every GLOBAL tree (levels of <= cnt / 2 entries) from the ranks' local tops
static int residue_tops(vpin_ctx* c, vpin::SparkForest& f, const DistPlan& pl, int npc, size_t cnt, const char* tag, std::vector<Fq>& tops) {
  const int W = pl.world;
  const size_t cntl = cnt / (size_t)W;
  int rc;
  if (cntl < 2 || cntl > f.stride()) return VPIN_ESHAPE;
  if ((rc = vpin::spark_fetch_tops(c, &f, cntl))) return rc;
  std::vector<Fq> all((size_t)npc * cntl * W);
  if ((rc = vpin::comm_allgather_ctx(c, c->h_spark, all.data(), (size_t)npc * cntl * 32, tag))) return rc;
  for (int t = 0; t < npc; t++) {
    Fq* g = &tops[(size_t)t * cnt];
    // levels of m >= W entries: global[i] = local_{i mod W}[i / W]; a level of m entries sits at offset cnt - 2m
    for (size_t m = cnt / 2; m >= (size_t)W; m >>= 1) {
      const size_t ml = m / W;
      for (size_t i = 0; i < m; i++) g[cnt - 2 * m + i] = all[((size_t)(i % W) * npc + t) * cntl + (cntl - 2 * ml) + i / W];
    }
    // the levels above: products of the level below (product_tree.rs:18-35)
    for (size_t m = (size_t)W / 2; m >= 1; m >>= 1)
      for (size_t i = 0; i < m; i++) g[cnt - 2 * m + i] = g[cnt - 4 * m + i] * g[cnt - 4 * m + m + i];
  }
  return VPIN_OK;
}

// Split by residue class: once every local table is one entry, the W entries of each table are gathered and the last
// lw rounds of the layer run here.  A, B per product circuit; L, R, W (D[0..2]) per dot-product half.
struct GatheredTables {
  std::vector<std::vector<Fq>> A, B, D[3];

  // fin: this rank's entry of every table, cl | cr per circuit and dp[3 i + tb] per half
  int gather(vpin_ctx* c, int W, int npc, bool with_dotp, const Fq* cl, const Fq* cr, const Fq* dp, const char* tag) {
    const size_t per_rank = 2 * (size_t)npc + (with_dotp ? 18 : 0);
    std::vector<Fq> mine(per_rank), all(per_rank * (size_t)W);
    for (int t = 0; t < npc; t++) { mine[2 * (size_t)t] = cl[t]; mine[2 * (size_t)t + 1] = cr[t]; }
    if (with_dotp) for (int x = 0; x < 18; x++) mine[2 * (size_t)npc + x] = dp[x];
    int rc = vpin::comm_allgather_ctx(c, mine.data(), all.data(), per_rank * 32, tag);
    if (rc) return rc;
    A.assign(npc, std::vector<Fq>(W)); B.assign(npc, std::vector<Fq>(W));
    for (int t = 0; t < npc; t++)
      for (int rk = 0; rk < W; rk++) { A[t][rk] = all[(size_t)rk * per_rank + 2 * t]; B[t][rk] = all[(size_t)rk * per_rank + 2 * t + 1]; }
    if (with_dotp)
      for (int tb = 0; tb < 3; tb++) {
        D[tb].assign(6, std::vector<Fq>(W));
        for (int i = 0; i < 6; i++)
          for (int rk = 0; rk < W; rk++) D[tb][i][rk] = all[(size_t)rk * per_rank + 2 * (size_t)npc + 3 * (size_t)i + tb];
      }
    return VPIN_OK;
  }
  // a round's sums in the kernels' conventions, single-GPU slot order; E = eq(rho_{j+1..}, .), len / 2 entries
  void round_sums(const Fq* rho_next, bool lead, bool with_dotp, Fq* res) const {
    const size_t len = A[0].size(), half = len / 2;
    std::vector<Fq> E(half);
    host_eq(rho_next, log2z(half), E.data());
    for (size_t t = 0; t < A.size(); t++) {
      Fq a0 = Fq::zero(), a1 = Fq::zero(), a2 = Fq::zero();
      for (size_t i = 0; i < half; i++) {
        const Fq A0 = A[t][i], dA = A[t][i + half] - A0, B0 = B[t][i], dB = B[t][i + half] - B0;
        if (lead) {
          a0 = a0 + E[i] * (A0 * B0);
          a1 = a1 + E[i] * (dA * dB);
        } else {
          const Fq A2 = A0 + dA + dA, B2 = B0 + dB + dB, A3 = A2 + dA, B3 = B2 + dB;
          a0 = a0 + E[i] * (A0 * B0); a1 = a1 + E[i] * (A2 * B2); a2 = a2 + E[i] * (A3 * B3);
        }
      }
      res[3 * t] = a0; res[3 * t + 1] = a1; res[3 * t + 2] = a2;
    }
    if (with_dotp)
      for (int i = 0; i < 6; i++) {
        Fq q0 = Fq::zero(), q2 = Fq::zero(), q3 = Fq::zero();
        for (size_t x = 0; x < half; x++) {
          Fq v0[3], v2[3], v3[3];
          for (int tb = 0; tb < 3; tb++) {
            const Fq p = D[tb][i][x], d = D[tb][i][x + half] - p;
            v0[tb] = p; v2[tb] = p + d + d; v3[tb] = v2[tb] + d;
          }
          q0 = q0 + v0[0] * v0[1] * v0[2]; q2 = q2 + v2[0] * v2[1] * v2[2]; q3 = q3 + v3[0] * v3[1] * v3[2];
        }
        Fq* q = res + 3 * (size_t)(kHalfSlot + i);
        q[0] = q0; q[1] = q2; q[2] = q3;
      }
  }
  // bound_poly_var_top
  void fold(const Fq& rj, bool with_dotp) {
    auto f1 = [&](std::vector<Fq>& T) {
      const size_t half = T.size() / 2;
      for (size_t i = 0; i < half; i++) T[i] = T[i] + rj * (T[i + half] - T[i]);
      T.resize(half);
    };
    for (size_t t = 0; t < A.size(); t++) { f1(A[t]); f1(B[t]); }
    if (with_dotp) for (int tb = 0; tb < 3; tb++) for (int i = 0; i < 6; i++) f1(D[tb][i]);
  }
};

// A layer of at most kSparkHostTop entries: prove_cubic_batched (sumcheck.rs:248-425) as written, on the tree tops.
// (The residue-class prover once summed with cc = s * eq(rand_j.., .) instead of folding C: the same field elements, since
// eq(rand, (x0, rest)) folded at r0 is eq1(rand_0, r0) * eq(rand_1.., rest).)
static void host_layer(Transcript& tr, const std::vector<Fq>& tops, size_t cnt, int npc, size_t h, int k, const std::vector<Fq>& rand,
                       const std::vector<Fq>& coeffs, Fq e, Fq* r, Fq* polys, Fq* cl, Fq* cr) {
  std::vector<Fq> C(h), A((size_t)npc * h), Bv((size_t)npc * h);
  host_eq(rand.data(), (size_t)k, C.data());
  for (int t = 0; t < npc; t++) {
    const Fq* lvl = &tops[(size_t)t * cnt + cnt - 4 * h];  // level of 2h entries
    memcpy(&A[(size_t)t * h], lvl, h * 32);
    memcpy(&Bv[(size_t)t * h], lvl + h, h * 32);
  }
  size_t len = h;
  for (int j = 0; j < k; j++) {
    const size_t half = len / 2;
    Fq c0 = Fq::zero(), c2 = Fq::zero(), c3 = Fq::zero();
    for (int t = 0; t < npc; t++) {
      const Fq* a = &A[(size_t)t * h];
      const Fq* b = &Bv[(size_t)t * h];
      Fq e0 = Fq::zero(), e2 = Fq::zero(), e3 = Fq::zero();
      for (size_t i = 0; i < half; i++) {
        e0 = e0 + a[i] * b[i] * C[i];
        Fq a2 = a[half + i] + a[half + i] - a[i], b2 = b[half + i] + b[half + i] - b[i], c2p = C[half + i] + C[half + i] - C[i];
        e2 = e2 + a2 * b2 * c2p;
        Fq a3 = a2 + a[half + i] - a[i], b3 = b2 + b[half + i] - b[i], c3p = c2p + C[half + i] - C[i];
        e3 = e3 + a3 * b3 * c3p;
      }
      c0 = c0 + e0 * coeffs[t]; c2 = c2 + e2 * coeffs[t]; c3 = c3 + e3 * coeffs[t];
    }
    Fq evals[4] = {c0, e - c0, c2, c3}, cf[4];
    unipoly_from_evals(evals, 4, cf);
    append_unipoly(tr, cf, 4);
    Fq rj = tr.challenge_scalar("challenge_nextround");
    r[j] = rj;
    for (int t = 0; t < npc; t++) {
      Fq* a = &A[(size_t)t * h];
      Fq* b = &Bv[(size_t)t * h];
      for (size_t i = 0; i < half; i++) { a[i] = a[i] + rj * (a[half + i] - a[i]); b[i] = b[i] + rj * (b[half + i] - b[i]); }
    }
    for (size_t i = 0; i < half; i++) C[i] = C[i] + rj * (C[half + i] - C[i]);
    e = unipoly_eval(cf, 4, rj);
    polys[3 * j] = cf[0]; polys[3 * j + 1] = cf[2]; polys[3 * j + 2] = cf[3];
    len = half;
  }
  for (int t = 0; t < npc; t++) { cl[t] = A[(size_t)t * h]; cr[t] = Bv[(size_t)t * h]; }
}

// The two live entries of every table after the last device round (spark_tail_final's layout: 6 scalars per instance, the
// halves from instance `hs` on) bound with that round's challenge: cl | cr per circuit, dp[3 i + tb] per half
static void bind_finals(const Fq* fin, const Fq& rl, int npc, bool with_dotp, int hs, Fq* cl, Fq* cr, Fq* dp) {
  for (int t = 0; t < npc; t++) {
    cl[t] = fin[6 * t] + rl * (fin[6 * t + 1] - fin[6 * t]);
    cr[t] = fin[6 * t + 2] + rl * (fin[6 * t + 3] - fin[6 * t + 2]);
  }
  if (with_dotp)
    for (int i = 0; i < 6; i++)
      for (int tb = 0; tb < 3; tb++) {
        const Fq* q = fin + 6 * (hs + i) + 2 * tb;
        dp[3 * i + tb] = q[0] + rl * (q[1] - q[0]);
      }
}

// One prover for the three ways a forest of npc circuits (12 ops / 4 mem) of n leaves each is held:
//   one GPU (pl == nullptr): `f` is the whole forest.
//   by circuit (pl, pl->lw == 0): `f` holds this rank's circuits only (possibly none: f.ncirc == 0) and the rank runs its own
//     dot-product halves; every per-round result is exchanged (dist_exchange).  A rank without circuits of this forest
//     only follows the transcript.
//   by residue class (pl->lw > 0, a power-of-two world W): `f` is this rank's local forest, all npc circuits with n / W leaves
//     each (local index i <-> global index rank + i W).  A layer of h = 2^k entries per half is 2^(k - lw) entries locally:
//     the first k - lw rounds run on the device exactly as on one GPU (same launches, same persistent tail, the suffix
//     pyramid of the first k - lw challenges), the rank's eq-factored sums are scaled by eq(rand_lo, rank) and added up over
//     the ranks (dist_sum); then every local table is one entry, the W entries of each table are gathered and the last lw
//     rounds run on the host (GatheredTables).
// The modes differ only in where a round's sums and a layer's final entries come from; the transcript work is the same on
// every rank.  Layers of at most kSparkHostTop entries are proven on the host from the tree tops (host_layer).
//
// Slot convention.  Everything the round algebra reads, and every exchanged or summed buffer, is in the single-GPU slot
// order: circuit t at slot t, dot-product half i at slot kHalfSlot + i (3 scalars per slot for a round's sums, 6 for the
// final entries).  A launch group (spark_prod_round + spark_dotp_round) writes h_spark in that order, a rank's own halves at
// kHalfSlot, kHalfSlot + 1, ..; the persistent tail numbers the instances it runs consecutively, circuits 0..nl-1 and the
// halves from nl on (the same thing on one GPU, where nl == 12 whenever halves ride along).  dist_exchange takes a rank's
// instances packed consecutively (circuits, then halves) and returns the slot order; the residue split sums slot-ordered buffers.
static int product_prove(vpin_ctx* c, vpin::SparkForest& f, int npc, DotpCtx* dotp, Transcript& tr, Batched& out, std::vector<Fq>& rand,
                         const DistPlan* pl) {
  const int ndotp = dotp ? 6 : 0, lw = pl ? pl->lw : 0;
  const bool by_circuit = pl && lw == 0, by_residue = lw > 0, is_mem = npc == 4;
  const size_t n = f.n << lw;                                         // leaves of a whole circuit
  const int nl = f.ncirc;                                             // circuits this rank runs
  const std::vector<int> no_halves;
  const std::vector<int>& my_halves = by_circuit ? pl->dotp_of[pl->rank] : no_halves;
  const int ndl = !dotp ? 0 : (by_circuit ? (int)my_halves.size() : 6);  // dot-product halves this rank runs
  const int* halves = by_circuit ? my_halves.data() : nullptr;
  static const bool fine = getenv("VPIN_SPARK_TRACE") && atoi(getenv("VPIN_SPARK_TRACE")) >= 2;
  double t_setup = 0, t_first = 0, t_rounds = 0, t_epi = 0, t_host = 0;
  auto tl0 = Clock::now();
  const int num_layers = (int)log2z(n);
  int rc;
  // host copies of the small top levels: the last cnt entries of every tree
  const size_t cnt = std::min<size_t>(2 * vpin::kSparkHostTop, 2 * n);
  std::vector<Fq> tops((size_t)npc * cnt, Fq::zero());
  const char* tops_tag = is_mem ? "mem_tops" : "ops_tops";
  if (by_residue) {
    if ((rc = residue_tops(c, f, *pl, npc, cnt, tops_tag, tops))) return rc;
  } else {
    if (nl && (rc = vpin::spark_fetch_tops(c, &f, cnt))) return rc;
    if (!pl) memcpy(tops.data(), c->h_spark, tops.size() * 32);
    else if ((rc = dist_exchange(c, *pl, is_mem, false, reinterpret_cast<const Fq*>(c->h_spark), (int)cnt, tops.data(), tops_tag))) return rc;
  }
  std::vector<Fq> res_all(3 * (size_t)vpin::kSparkMaxInst), fin_all(6 * (size_t)vpin::kSparkMaxInst), pack(6 * (size_t)vpin::kSparkMaxInst);

  struct TailGuard { vpin_ctx* c; ~TailGuard() { vpin::spark_tail_abort(c); } } tail_guard{c};  // a no-op unless an error return leaves a tail resident
  out.polys.assign(num_layers, {});
  out.claims_left.assign(num_layers, {});
  out.claims_right.assign(num_layers, {});
  std::vector<Fq> claims(npc + ndotp), coeffs;
  for (int t = 0; t < npc; t++) claims[t] = tops[(size_t)t * cnt + cnt - 2];  // the root: ProductCircuit::evaluate
  rand.clear();
  TableGuard tg(c);
  EqRound rd;

  for (int layer_id = num_layers - 1, o = 0; layer_id >= 0; layer_id--, o++) {
    const size_t h = n >> (layer_id + 1);    // entries of left_vec[layer_id]
    const int k = (int)log2z(h);             // rounds; rand.size() == k
    const bool with_dotp = (layer_id == 0 && ndotp > 0);
    int nclaims = npc;
    if (with_dotp) {
      for (int i = 0; i < 6; i++) claims[npc + i] = dotp->claims[i];
      nclaims += 6;
    }
    if (fine) tl0 = Clock::now();
    coeffs = tr.challenge_vector("rand_coeffs_next_layer", nclaims);
    Fq e = Fq::zero();
    for (int i = 0; i < nclaims; i++) e = e + claims[i] * coeffs[i];
    std::vector<Fq> r(k);
    std::vector<Fq>& polys = out.polys[o];
    polys.resize(3 * (size_t)k);
    std::vector<Fq> cl(npc), cr(npc);
    Fq dp[18];  // the halves' final entries, dp[3 i + tb]
    const bool on_host = (2 * h <= vpin::kSparkHostTop) && layer_id != 0;

    if (on_host) {
      host_layer(tr, tops, cnt, npc, h, k, rand, coeffs, e, r.data(), polys.data(), cl.data(), cr.data());
    } else {
      const int kl = k - lw;                             // rounds on the device
      const size_t hl = h >> lw;                         // entries per half on this rank
      if (by_residue && kl < 1) {  // (a zero challenge is refused with the tail below)
        vpin::set_last_error("split by residue class: layer too small for the world, or a zero challenge", hipErrorUnknown);
        return VPIN_ESHAPE;
      }
      if (k < 1) return VPIN_ESHAPE;
      const int ndl_here = with_dotp ? ndl : 0;          // halves this rank runs on this layer
      const bool runs = nl > 0 || ndl_here > 0;          // a rank without circuits of this forest only follows the transcript
      vpin_table* pyr = nullptr;
      if (runs) {
        if ((rc = vpin_eq_suffix_tables(c, B(rand.data()), kl, &pyr))) return rc;
        tg.add(pyr);
      }
      rd.begin(rand.data(), k, claims.data(), coeffs.data(), npc);
      Fq c_rank = Fq::one();  // by residue: eq(rand_lo, rank), the scale of this rank's eq-factored sums
      if (by_residue) {
        std::vector<Fq> eq_lo((size_t)pl->world);
        host_eq(rand.data() + kl, (size_t)lw, eq_lo.data());
        c_rank = eq_lo[pl->rank];
      }
      // Rounds with at most spark_tail_pairs() pairs per circuit are proven by ONE resident launch (spark.hip, persistent
      // tail): the kernel publishes a round's sums to pinned memory and polls a pinned mailbox for the challenge this
      // loop derives from the transcript.  Larger rounds take one launch each.
      const size_t tail_pairs = rd.lead_ok ? vpin::spark_tail_pairs() : 0;
      if (pl && tail_pairs == 0) {  // the split rounds end in the persistent tail; a zero challenge (never) or VPIN_SPARK_TAIL_PAIRS=0 rules it out
        vpin::set_last_error("one proof over several GPUs needs the persistent tail rounds", hipErrorUnknown);
        return VPIN_ESHAPE;
      }
      bool tail_on = false;
      int tail_j0 = 0;
      const int ninst = nl + ndl_here;  // instances this rank's launches carry
      GatheredTables gt;
      if (fine) { auto t = Clock::now(); t_setup += secs(tl0, t); tl0 = t; }
      for (int j = 0; j < k; j++) {
        const Fq* res = nullptr;
        if (j < kl) {
          // ---- a device round on this rank's tables ----
          const size_t len = j == 0 ? hl : (hl >> (j - 1));  // live length before this round's launch
          const uint8_t* rprev = j ? B(&r[j - 1]) : nullptr;
          if (!tail_on && (hl >> (j + 1)) <= tail_pairs) {
            if (runs && (rc = vpin::spark_tail_launch(c, &f, layer_id, kl, j, len, pyr->d, rprev, ndl_here ? dotp->N : 0,
                                                      ndl_here ? dotp->vals : nullptr, ndl_here ? dotp->derefs : nullptr,
                                                      ndl_here ? dotp->scratch : nullptr, halves, ndl_here)))
              return rc;
            tail_on = true;
            tail_j0 = j;
          }
          if (tail_on) {
            if (runs) {
              if ((rc = vpin::spark_tail_wait(c, j - tail_j0, ninst, nl))) return rc;
              res = reinterpret_cast<const Fq*>(vpin::spark_tail_sums(c));
            }
          } else if (runs) {
            const vpin::fq* E = pyr->d + vpin::pyramid_offset(kl, j + 1);
            if ((rc = vpin::spark_prod_round(c, &f, layer_id, len, E, rprev, ndl_here, rd.lead_ok))) return rc;
            if (ndl_here && (rc = vpin::spark_dotp_round(c, dotp->N, dotp->vals, dotp->derefs, dotp->scratch, len, j == 1, rprev, halves, ndl_here))) return rc;
            if ((rc = vpin::spark_wait_flag(c))) return rc;
            res = reinterpret_cast<const Fq*>(c->h_spark);
          }
          const int hs = tail_on ? nl : kHalfSlot;  // where this rank's halves start in res
          if (by_circuit) {
            // this rank's sums, packed -> everyone's, in the slot order
            for (int t = 0; t < nl; t++) memcpy(&pack[3 * (size_t)t], res + 3 * (size_t)t, 96);
            for (int i = 0; i < ndl_here; i++) memcpy(&pack[3 * (size_t)(nl + i)], res + 3 * (size_t)(hs + i), 96);
            if ((rc = dist_exchange(c, *pl, is_mem, with_dotp, pack.data(), 3, res_all.data(),
                                    is_mem ? (tail_on ? "mem_tail_round" : "mem_round") : (tail_on ? "ops_tail_round" : "ops_round"))))
              return rc;
            res = res_all.data();
          } else if (by_residue) {
            // this rank's share of every sum: the circuits' scaled by c_rank, the halves' as they are (no eq factor)
            for (int x = 0; x < 3 * npc; x++) pack[x] = res[x] * c_rank;
            if (with_dotp) memcpy(&pack[3 * (size_t)kHalfSlot], res + 3 * (size_t)hs, 6 * 96);
            if ((rc = dist_sum(c, *pl, pack.data(), with_dotp ? 3 * (size_t)vpin::kSparkMaxInst : 3 * (size_t)npc, res_all.data(),
                               is_mem ? "mem_round" : "ops_round")))
              return rc;
            res = res_all.data();
          }
        } else {
          // ---- by residue: a host round on the gathered tables ----
          gt.round_sums(rand.data() + j + 1, rd.lead_ok, with_dotp, res_all.data());
          res = res_all.data();
        }
        if (fine) { auto t = Clock::now(); (j == 0 ? t_first : t_rounds) += secs(tl0, t); if (k >= 11) fprintf(stderr, " w%.1f", secs(tl0, t) * 1e6); tl0 = t; }
        const Fq* cf = rd.combine(res, coeffs.data(), npc, with_dotp, e);
        append_unipoly(tr, cf, 4);
        Fq rj = tr.challenge_scalar("challenge_nextround");
        if (tail_on && runs && j + 1 < kl) vpin::spark_tail_reply(c, j - tail_j0, B(&rj));  // the kernel folds while the host finishes the round
        r[j] = rj;
        rd.advance(rj, e);
        polys[3 * j] = cf[0]; polys[3 * j + 1] = cf[2]; polys[3 * j + 2] = cf[3];
        if (j >= kl) {
          gt.fold(rj, with_dotp);
        } else if (by_residue && j + 1 == kl) {
          // the device rounds are over: the two live entries of every local table, bound with r_j, are this rank's entry of
          // the W-entry tables the remaining rounds run on
          bind_finals(reinterpret_cast<const Fq*>(vpin::spark_tail_final(c)), rj, npc, with_dotp, nl, cl.data(), cr.data(), dp);
          vpin::spark_tail_end(c);
          if ((rc = gt.gather(c, pl->world, npc, with_dotp, cl.data(), cr.data(), dp, is_mem ? "mem_gather_tables" : "ops_gather_tables")))
            return rc;
        }
        if (fine) { auto t = Clock::now(); t_host += secs(tl0, t); if (k >= 11) fprintf(stderr, " m%.1f", secs(tl0, t) * 1e6); tl0 = t; }
      }
      if (fine && k >= 11) fprintf(stderr, "\n");
      // the layer's final entries: the two live entries per table folded with r_{k-1}
      const Fq rl = r[k - 1];
      if (by_residue) {
        for (int t = 0; t < npc; t++) { cl[t] = gt.A[t][0]; cr[t] = gt.B[t][0]; }
        if (with_dotp)
          for (int i = 0; i < 6; i++)
            for (int tb = 0; tb < 3; tb++) dp[3 * i + tb] = gt.D[tb][i][0];
      } else if (tail_on) {
        const Fq* fin = runs ? reinterpret_cast<const Fq*>(vpin::spark_tail_final(c)) : nullptr;
        if (by_circuit) {
          for (int t = 0; t < ninst; t++) memcpy(&pack[6 * (size_t)t], fin + 6 * (size_t)t, 192);  // the tail numbers its instances 0..ninst-1
          if ((rc = dist_exchange(c, *pl, is_mem, with_dotp, pack.data(), 6, fin_all.data(), is_mem ? "mem_finals" : "ops_finals"))) return rc;
          fin = fin_all.data();
        }
        bind_finals(fin, rl, npc, with_dotp, kHalfSlot, cl.data(), cr.data(), dp);  // (halves ride along only with npc == 12 == kHalfSlot)
        if (runs) vpin::spark_tail_end(c);
      } else {
        // launch-only end of a layer (VPIN_SPARK_TAIL_PAIRS=0, or a zero challenge): one GPU only
        if (pl) return VPIN_ESHAPE;
        if ((rc = vpin::spark_collect(c, &f, layer_id, with_dotp ? dotp->d : nullptr, with_dotp ? dotp->derefs : nullptr,
                                      with_dotp ? dotp->scratch : nullptr, with_dotp, k >= 2)))
          return rc;
        const Fq* res = reinterpret_cast<const Fq*>(c->h_spark);
        for (int t = 0; t < npc; t++) {
          cl[t] = res[4 * t] + rl * (res[4 * t + 1] - res[4 * t]);
          cr[t] = res[4 * t + 2] + rl * (res[4 * t + 3] - res[4 * t + 2]);
        }
        if (with_dotp) {
          const Fq* q = reinterpret_cast<const Fq*>(c->h_spark) + 64;
          for (int i = 0; i < 6; i++)
            for (int t = 0; t < 3; t++) dp[3 * i + t] = q[6 * i + 2 * t] + rl * (q[6 * i + 2 * t + 1] - q[6 * i + 2 * t]);
        }
      }
    }

    for (int t = 0; t < npc; t++) {
      tr.append_scalar("claim_prod_left", cl[t]);
      tr.append_scalar("claim_prod_right", cr[t]);
    }
    if (with_dotp) {
      for (int t = 0; t < 3; t++) out.dotp[t].resize(6);
      for (int i = 0; i < 6; i++) {
        for (int t = 0; t < 3; t++) out.dotp[t][i] = dp[3 * i + t];
        tr.append_scalar("claim_dotp_left", out.dotp[0][i]);
        tr.append_scalar("claim_dotp_right", out.dotp[1][i]);
        tr.append_scalar("claim_dotp_weight", out.dotp[2][i]);
      }
    }
    Fq r_layer = tr.challenge_scalar("challenge_r_layer");
    for (int t = 0; t < npc; t++) claims[t] = cl[t] + r_layer * (cr[t] - cl[t]);
    out.claims_left[o] = cl;
    out.claims_right[o] = cr;
    std::vector<Fq> ext;
    ext.reserve(k + 1);
    ext.push_back(r_layer);
    ext.insert(ext.end(), r.begin(), r.end());
    rand.swap(ext);
    if (fine) { auto t = Clock::now(); t_epi += secs(tl0, t); tl0 = t; }
  }
  if (fine)
    fprintf(stderr, "[spark]   forest of %d x 2^%d: setup %.3f  first result %.3f  later results %.3f  host per-round math %.3f  epilogue %.3f ms\n",
            npc, num_layers, t_setup * 1e3, t_first * 1e3, t_rounds * 1e3, t_host * 1e3, t_epi * 1e3);
  return VPIN_OK;
}

static thread_local double g_spark_timings[8];

// split by whole circuits: each of `cnt` scalars comes from the one rank that computed it (owner[i]; the others send zero)
static int dist_pick(vpin_ctx* c, const DistPlan& pl, const Fq* mine, size_t cnt, const int* owner, Fq* out, const char* tag) {
  std::vector<Fq> all(cnt * (size_t)pl.world);
  int rc = vpin::comm_allgather_ctx(c, mine, all.data(), cnt * 32, tag);
  if (rc) return rc;
  for (size_t i = 0; i < cnt; i++) out[i] = all[cnt * (size_t)owner[i] + i];
  return VPIN_OK;
}

// One SparseMatPolyEvalProof::prove in flight: what the stages below (one per timing slot) hand to each other.  The three
// configurations -- one GPU (!dz), split by whole circuits (dz && !st), split by residue class (st) -- are plain branches
// inside the stages.
struct SparkProof {
  vpin_ctx* c;
  const vpin_spark_decomm* d;
  const std::vector<Fq>&rx, &ry;
  const Fq* evals;
  Transcript &tr, &tape;
  const size_t N, M, lgN, lgM;
  const PcGens *g_ops = nullptr, *g_mem = nullptr, *g_derefs = nullptr;
  TableGuard tg;
  // one proof over several GPUs (vpin_ctx_set_comm): every rank is here with the same transcript state
  DistPlan plan;
  const DistPlan* dz = nullptr;
  bool st = false;                  // split by residue class
  vpin::SparkLeaves leaves;         // the entries this rank holds of every circuit and committed polynomial: all, or (rank, world)
  size_t Nf = 0, Mf = 0;            // leaves per tree on this rank
  bool defer_mem = false;
  // derefs: the whole polynomial (comb), or -- split by residue class -- the local views (spark.hip) and a shape-only handle
  vpin_table *mem_rx = nullptr, *mem_ry = nullptr, *comb = nullptr;
  vpin_table comb_shape;
  vpin::DevBuf b_cloc, b_crows, b_vloc, b_ops, b_mem, b_scr;
  vpin::fq* comb_rows = nullptr;
  const vpin::fq *derefs = nullptr, *vals = nullptr;  // the six derefs slices and the three val slices over `leaves`
  std::vector<CG> comm_derefs;
  vpin::HashParams hash;
  vpin::SparkForest f_ops, f_mem;
  Fq pl[2][8];  // roots per side: init, read[3], write[3], audit
  DotpCtx dotp;
  Fq dotp_left[3], dotp_right[3];
  Batched pf_ops, pf_mem;
  std::vector<Fq> rand_ops, rand_mem;
  Fq ev_derefs[6], ev_ops[15], ev_mem[2];
  DpLog pe_derefs, pe_ops, pe_mem;
  // a whole SNARK on one GPU (spark_inst_evals): the derefs pass and the six dot-product sums ran before the sat proof's last
  // transcript appends, which need their sums; stage_derefs and dotp_claims take them from here
  bool have_derefs = false, have_sums = false;
  Fq sums6[6];

  SparkProof(vpin_ctx* c_, const vpin_spark_decomm* d_, const std::vector<Fq>& rx_, const std::vector<Fq>& ry_, const Fq* evals_,
             Transcript& tr_, Transcript& tape_)
      : c(c_), d(d_), rx(rx_), ry(ry_), evals(evals_), tr(tr_), tape(tape_), N(d_->N), M(d_->M), lgN(log2z(d_->N)), lgM(log2z(d_->M)),
        tg(c_), b_cloc(c_), b_crows(c_), b_vloc(c_), b_ops(c_), b_mem(c_), b_scr(c_) {}
  bool by_circuit() const { return dz && !st; }
};

static int split_plan(SparkProof& S) {
  vpin_ctx* c = S.c;
  if (!(c->comm && c->comm->world > 1)) return VPIN_OK;
  if (c->comm->world > 12) return VPIN_EINVAL;  // every rank owns at least one of the 12 ops circuits
  plan_init(S.plan, c->comm);
  S.dz = &S.plan;
  // a power-of-two world splits every circuit by residue class (product_prove: perfectly balanced, and the derefs
  // gather, the leaves and the slices shrink with the world too); otherwise the circuits are dealt out whole
  static const bool by_circuit = getenv("VPIN_DIST_BY_CIRCUIT") != nullptr;
  const size_t Wz = (size_t)S.plan.world;
  if (!by_circuit && (Wz & (Wz - 1)) == 0 && Wz <= 16 && S.N / Wz >= 4096 && S.M / Wz >= 4096 && S.g_derefs->L >= Wz)
    S.plan.lw = (int)log2z(Wz);
  S.st = S.plan.lw > 0;
  if (S.st) { S.leaves.r0 = (size_t)S.plan.rank; S.leaves.step = Wz; }
  return VPIN_OK;
}

// The two memories and the derefs polynomial (sparse_mlpoly.rs:525-531,56-71): a function of rx, ry and the circuit alone, not
// of the transcript
static int derefs_tables(SparkProof& S) {
  vpin_ctx* c = S.c;
  const vpin_spark_decomm* d = S.d;
  const DistPlan* dz = S.dz;
  const PcGens* g_derefs = S.g_derefs;
  const size_t N = S.N;
  int rc;
  // equalize (sparse_mlpoly.rs:1448-1465) + the two memories eq(rx_ext, .), eq(ry_ext, .)
  const size_t nm = std::max(d->nx, d->ny);
  std::vector<Fq> rx_ext(nm, Fq::zero()), ry_ext(nm, Fq::zero());
  std::copy(S.rx.begin(), S.rx.end(), rx_ext.begin() + (nm - d->nx));
  std::copy(S.ry.begin(), S.ry.end(), ry_ext.begin() + (nm - d->ny));
  if ((rc = vpin_eq_table(c, B(rx_ext.data()), (int)nm, &S.mem_rx))) return rc;
  S.tg.add(S.mem_rx);
  if ((rc = vpin_eq_table(c, B(ry_ext.data()), (int)nm, &S.mem_ry))) return rc;
  S.tg.add(S.mem_ry);
  const vpin::fq *mem_rx = S.mem_rx->d, *mem_ry = S.mem_ry->d;
  S.Nf = N / S.leaves.step; S.Mf = S.M / S.leaves.step;
  if (S.st) {
    S.comb_shape.d = nullptr; S.comb_shape.len = S.comb_shape.cap = 8 * N; S.comb_shape.owned = false;
    S.comb = &S.comb_shape;  // never materialised
    const size_t Nl = S.Nf, nrows_loc = vpin::comm_strided_count(g_derefs->L, dz->rank, dz->world);
    if (S.b_cloc.alloc(6 * Nl * 32) || S.b_crows.alloc(std::max<size_t>(1, nrows_loc) * g_derefs->R * 32) || S.b_vloc.alloc(3 * Nl * 32)) return VPIN_ENOMEM;
    S.comb_rows = (vpin::fq*)S.b_crows.p;
    if ((rc = vpin::spark_gather_derefs(c, d, S.leaves, mem_rx, mem_ry, (vpin::fq*)S.b_cloc.p, S.comb_rows, g_derefs->R, nrows_loc))) return rc;
    for (int m = 0; m < 3; m++)
      if ((rc = vpin::spark_take_strided(c, d->vals + (size_t)m * N, Nl, S.leaves.r0, S.leaves.step, (vpin::fq*)S.b_vloc.p + (size_t)m * Nl))) return rc;
    S.derefs = (const vpin::fq*)S.b_cloc.p; S.vals = (const vpin::fq*)S.b_vloc.p;
  } else {
    if ((rc = vpin::table_alloc_uninit(c, 8 * N, &S.comb))) return rc;
    S.tg.add(S.comb);
    if ((rc = vpin::spark_gather_derefs(c, d, S.leaves, mem_rx, mem_ry, S.comb->d))) return rc;
    S.derefs = S.comb->d; S.vals = d->vals;
  }
  S.have_derefs = true;
  return VPIN_OK;
}

// Derefs and their commitment
static int stage_derefs(SparkProof& S) {
  vpin_ctx* c = S.c;
  const vpin_spark_decomm* d = S.d;
  const DistPlan* dz = S.dz;
  const PcGens* g_derefs = S.g_derefs;
  const size_t N = S.N;
  int rc;
  S.tr.append_protocol_name("Sparse polynomial evaluation proof");
  if (!S.have_derefs && (rc = derefs_tables(S))) return rc;
  const vpin::fq* mem_ry = S.mem_ry->d;
  if ((rc = vpin::comm_mark(c, "derefs_gather"))) return rc;
  std::vector<CG>& comm_derefs = S.comm_derefs;
  // the entries of each matrix's hot column hold one scalar, E_ry[hot]: one addition each instead of a table walk
  const bool hot = d->hot_col[0] != 0xffffffffu || d->hot_col[1] != 0xffffffffu || d->hot_col[2] != 0xffffffffu;
  const uint32_t* col_idx[3] = {d->idx + 6 * N, d->idx + 7 * N, d->idx + 8 * N};
  if (dz) {
    // the L row commitments are independent MSMs over shared generators: rank r commits rows r, r + world, .. (the rows
    // differ in cost: two of the polynomial's eight slices are zero padding, the col slices carry the hot columns), 32
    // bytes per row are all-gathered (no point crosses a link, nothing is reduced)
    const size_t L = g_derefs->L, pmax = vpin::comm_block_max(L, dz->world);
    const size_t nrows = vpin::comm_strided_count(L, dz->rank, dz->world);  // rows rank, rank + world, ..
    std::vector<uint8_t> mine(pmax * 32, 0), all(pmax * 32 * (size_t)dz->world);
    if (nrows) {
      if (hot)
        rc = vpin::hyrax_commit_derefs_hot(c, g_derefs->dev, S.comb, L, N, col_idx, d->hot_col, mem_ry, mine.data(), (size_t)dz->rank,
                                           nrows, (size_t)dz->world, S.comb_rows);
      else
        rc = vpin::hyrax_commit_rows_strided(c, g_derefs->dev, S.comb, L, (size_t)dz->rank, nrows, (size_t)dz->world, mine.data(), S.comb_rows);
      if (rc) return rc;
    }
    if ((rc = vpin::comm_allgather_ctx(c, mine.data(), all.data(), mine.size(), "derefs_commit"))) return rc;
    comm_derefs.resize(L);
    for (int r = 0; r < dz->world; r++) {
      const size_t n = vpin::comm_strided_count(L, r, dz->world);
      for (size_t k = 0; k < n; k++) memcpy(comm_derefs[(size_t)r + k * (size_t)dz->world].b, all.data() + ((size_t)r * pmax + k) * 32, 32);
    }
  } else if (hot) {
    comm_derefs.resize(g_derefs->L);
    if ((rc = vpin::hyrax_commit_derefs_hot(c, g_derefs->dev, S.comb, g_derefs->L, N, col_idx, d->hot_col, mem_ry, comm_derefs[0].b))) return rc;
  } else if ((rc = commit_noblind(c, g_derefs, S.comb, comm_derefs))) {
    return rc;
  }
  S.tr.append_message("derefs_commitment", "begin_derefs_commitment");  // DerefsCommitment::append_to_transcript (:216-222)
  append_polycomm(S.tr, "comm_poly_row_col_ops_val", comm_derefs);
  S.tr.append_message("derefs_commitment", "end_derefs_commitment");
  return VPIN_OK;
}

static vpin::HashParams make_hash(const Fq& r_hash, const Fq& gamma) {
  const Fq r2 = r_hash * r_hash, r2_boost = r2 * Fq::r2();
  vpin::HashParams hp;
  memcpy(hp.r.v, B(&r_hash), 32); memcpy(hp.r2.v, B(&r2), 32); memcpy(hp.r2_boost.v, B(&r2_boost), 32); memcpy(hp.gamma.v, B(&gamma), 32);
  return hp;
}

// PolyEvalNetwork::new (sparse_mlpoly.rs:681-696)
static int stage_network(SparkProof& S) {
  vpin_ctx* c = S.c;
  const DistPlan* dz = S.dz;
  int rc;
  std::vector<Fq> r_mem_check = S.tr.challenge_vector("challenge_r_hash", 2);
  S.hash = make_hash(r_mem_check[0], r_mem_check[1]);
  // which leaves this rank builds: S.leaves of all 12 + 4 circuits, or -- split by whole circuits -- every leaf of its own
  vpin::SparkLeaves lv_ops = S.leaves, lv_mem = S.leaves;
  int nl_ops = 12, nl_mem = 4;
  size_t nl_dotp = 6;  // the first-fold scratch is numbered by the local half
  if (S.by_circuit()) {
    const auto &ops = dz->ops_of[dz->rank], &mem = dz->mem_of[dz->rank];
    lv_ops.ncirc = nl_ops = (int)ops.size(); lv_mem.ncirc = nl_mem = (int)mem.size();
    std::copy(ops.begin(), ops.end(), lv_ops.ids);
    std::copy(mem.begin(), mem.end(), lv_mem.ids);
    nl_dotp = dz->dotp_of[dz->rank].size();
  }
  // Single GPU, a context in low-memory mode (vpin_ctx_set_low_memory, or VPIN_MEM_FOREST_LATE=1; round 5): the mem forest is
  // built AFTER the ops forest has been proven, into the memory it frees (-16 GiB of working set for the 2^25 instance, the
  // LeNet step's HBM 197 -> 181 GiB); the four mem roots the transcript wants first come from a product reduction over the
  // leaves (spark_mem_roots).  It costs 1 % of the 2^25 proof and 1.6 % of the four-lane step, so it is not the default.
  S.defer_mem = !dz && (c->low_memory || getenv("VPIN_MEM_FOREST_LATE") != nullptr);
  if (S.b_ops.alloc((size_t)nl_ops * 2 * S.Nf * 32) || (nl_mem && !S.defer_mem && S.b_mem.alloc((size_t)nl_mem * 2 * S.Mf * 32)) ||
      S.b_scr.alloc(std::max<size_t>(256, 3 * nl_dotp * (S.Nf / 4) * 32)))
    return VPIN_ENOMEM;
  if ((rc = vpin::comm_mark(c, "network_alloc"))) return rc;
  S.f_ops.base = (vpin::fq*)S.b_ops.p; S.f_ops.n = S.Nf; S.f_ops.ncirc = nl_ops;
  S.f_mem.base = (vpin::fq*)S.b_mem.p; S.f_mem.n = S.Mf; S.f_mem.ncirc = nl_mem;
  const vpin::SparkInputs in{S.derefs, S.mem_rx->d, S.mem_ry->d};
  if (!S.by_circuit() && !S.defer_mem) {
    rc = vpin::spark_build_forests(c, S.d, S.hash, S.leaves, in, &S.f_ops, &S.f_mem);
  } else {
    rc = vpin::spark_build_forest(c, S.d, S.hash, lv_ops, in, &S.f_ops, false);
    if (!rc && !S.defer_mem && nl_mem) rc = vpin::spark_build_forest(c, S.d, S.hash, lv_mem, in, &S.f_mem, true);
  }
  if (rc || (rc = vpin::spark_wait(c))) return rc;
  return vpin::comm_mark(c, "network_build");
}

// roots of the 16 circuits -> S.pl and the transcript
static int product_roots(SparkProof& S) {
  vpin_ctx* c = S.c;
  const DistPlan* dz = S.dz;
  const bool st = S.st;
  const size_t Wz = S.leaves.step;
  auto& pl = S.pl;
  int rc;
  {
    std::vector<Fq> roots(2 * (size_t)vpin::kSparkMaxInst);
    if ((rc = vpin::spark_fetch_tops(c, &S.f_ops, 2))) return rc;
    const Fq* t = reinterpret_cast<const Fq*>(c->h_spark);
    std::vector<Fq> st_roots(2 * 16);
    if (st) {
      // a circuit's root is the product of its leaves = the product over the ranks of their local roots
      std::vector<Fq> mine16(16), all16(16 * Wz);
      for (int i = 0; i < 12; i++) mine16[i] = t[2 * i];
      if ((rc = vpin::spark_fetch_tops(c, &S.f_mem, 2))) return rc;
      for (int i = 0; i < 4; i++) mine16[12 + i] = t[2 * i];
      if ((rc = vpin::comm_allgather_ctx(c, mine16.data(), all16.data(), 16 * 32, "roots"))) return rc;
      for (int i = 0; i < 16; i++) {
        Fq p = Fq::one();
        for (size_t r = 0; r < Wz; r++) p = p * all16[16 * r + i];
        st_roots[2 * i] = p;
      }
      for (int i = 0; i < 12; i++) roots[2 * i] = st_roots[2 * i];
      t = roots.data();
    } else if (dz) {
      if ((rc = dist_exchange(c, *dz, false, false, t, 2, roots.data(), "roots"))) return rc;
      t = roots.data();
    }
    for (int s = 0; s < 2; s++)
      for (int m = 0; m < 3; m++) { pl[s][1 + m] = t[2 * (s * 6 + m)]; pl[s][4 + m] = t[2 * (s * 6 + 3 + m)]; }
    if (st) {
      for (int i = 0; i < 4; i++) roots[2 * i] = st_roots[2 * (12 + i)];
      t = roots.data();
    } else {
      if (S.defer_mem) {
        if ((rc = vpin::spark_mem_roots(c, S.d, S.hash, S.mem_rx->d, S.mem_ry->d))) return rc;
      } else if (S.f_mem.ncirc && (rc = vpin::spark_fetch_tops(c, &S.f_mem, 2))) {
        return rc;
      }
      t = reinterpret_cast<const Fq*>(c->h_spark);
      if (dz) {
        if ((rc = dist_exchange(c, *dz, true, false, t, 2, roots.data(), "roots"))) return rc;
        t = roots.data();
      }
    }
    for (int s = 0; s < 2; s++) { pl[s][0] = t[2 * (2 * s)]; pl[s][7] = t[2 * (2 * s + 1)]; }
  }
  static const char* lab[2][4] = {{"claim_row_eval_init", "claim_row_eval_read", "claim_row_eval_write", "claim_row_eval_audit"},
                                  {"claim_col_eval_init", "claim_col_eval_read", "claim_col_eval_write", "claim_col_eval_audit"}};
  for (int s = 0; s < 2; s++) {
    Fq ws = Fq::one(), rs = Fq::one();
    for (int m = 0; m < 3; m++) { rs = rs * pl[s][1 + m]; ws = ws * pl[s][4 + m]; }
    if (!(pl[s][0] * ws == rs * pl[s][7])) return VPIN_ESHAPE;  // assert_eq!(row_eval_init * ws, rs * row_eval_audit)
    S.tr.append_scalar(lab[s][0], pl[s][0]);
    S.tr.append_scalars(lab[s][1], &pl[s][1], 3);
    S.tr.append_scalars(lab[s][2], &pl[s][4], 3);
    S.tr.append_scalar(lab[s][3], pl[s][7]);
  }
  return VPIN_OK;
}

// DotProductCircuit::evaluate (product_tree.rs:87-91) of the six halves -> S.dotp.claims and the transcript
static int dotp_claims(SparkProof& S) {
  vpin_ctx* c = S.c;
  const DistPlan* dz = S.dz;
  int rc;
  // one GPU: all six halves.  Split by residue class: every rank sums its residue class of all six, the partial sums are added
  // up.  Split by whole circuits: every rank sums the halves it will prove, one scalar per half is exchanged.
  const std::vector<int>* hv = S.by_circuit() ? &dz->dotp_of[dz->rank] : nullptr;
  const size_t nh = hv ? hv->size() : 6;
  Fq mine6[6] = {};
  if (S.have_sums) {  // one GPU, all six: taken by spark_inst_evals
    std::copy(S.sums6, S.sums6 + 6, mine6);
  } else {
    if (nh && (rc = vpin::spark_triple_sums(c, S.derefs, S.vals, S.Nf, hv ? hv->data() : nullptr, (int)nh))) return rc;
    for (size_t i = 0; i < nh; i++) mine6[hv ? (*hv)[i] : i] = reinterpret_cast<const Fq*>(c->h_spark)[3 * i];
  }
  if (S.st) rc = dist_sum(c, *dz, mine6, 6, S.dotp.claims, "triple_sums");
  else if (dz) rc = dist_pick(c, *dz, mine6, 6, dz->owner_dotp, S.dotp.claims, "triple_sums");
  else std::copy(mine6, mine6 + 6, S.dotp.claims);
  if (rc) return rc;
  for (int m = 0; m < 3; m++) {
    S.dotp_left[m] = S.dotp.claims[2 * m];
    S.dotp_right[m] = S.dotp.claims[2 * m + 1];
    S.tr.append_scalar("claim_eval_dotp_left", S.dotp_left[m]);
    S.tr.append_scalar("claim_eval_dotp_right", S.dotp_right[m]);
    if (!(S.dotp_left[m] + S.dotp_right[m] == S.evals[m])) return VPIN_ESHAPE;  // assert_eq!(left + right, eval[i])
  }
  return VPIN_OK;
}

// PolyEvalNetworkProof::prove / ProductLayerProof::prove (:1336-1370, :1049-1227)
static int stage_product(SparkProof& S) {
  vpin_ctx* c = S.c;
  int rc;
  S.tr.append_protocol_name("Sparse polynomial evaluation proof");
  S.tr.append_protocol_name("Sparse polynomial product layer proof");
  if ((rc = product_roots(S))) return rc;
  S.dotp = DotpCtx{S.d, S.Nf, S.vals, S.derefs, (vpin::fq*)S.b_scr.p, {}};
  if ((rc = dotp_claims(S))) return rc;
  {
    TraceSpan ts("product: ops forest");
    if ((rc = product_prove(c, S.f_ops, 12, &S.dotp, S.tr, S.pf_ops, S.rand_ops, S.dz))) return rc;
  }
  if (S.defer_mem) {
    TraceSpan ts("network: mem forest (deferred)");
    S.b_ops.release();   // every level of the ops forest has been folded away: its memory takes the mem forest
    S.b_scr.release();
    if (S.b_mem.alloc((size_t)4 * 2 * S.M * 32)) return VPIN_ENOMEM;
    S.f_mem.base = (vpin::fq*)S.b_mem.p;
    if ((rc = vpin::spark_build_forest(c, S.d, S.hash, S.leaves, {nullptr, S.mem_rx->d, S.mem_ry->d}, &S.f_mem, true))) return rc;
    if ((rc = vpin::spark_wait(c))) return rc;
  }
  TraceSpan ts("product: mem forest");
  return product_prove(c, S.f_mem, 4, nullptr, S.tr, S.pf_mem, S.rand_mem, S.dz);
}

// One proof over several GPUs: the 23 DensePolynomial::evaluate of the hash layer (6 derefs + 15 ops slices against
// eq(rand_ops), 2 mem slices against eq(rand_mem)) -> S.ev_derefs | S.ev_ops | S.ev_mem.  They depend on nothing the
// transcript produces in between.
static int hash_slice_evals_dist(SparkProof& S, const vpin_table* comb_ops, const vpin_table* comb_mem, const vpin_table* eq_ops,
                                 const vpin_table* eq_mem) {
  vpin_ctx* c = S.c;
  const DistPlan* dz = S.dz;
  const size_t N = S.N, M = S.M;
  const Fq* hs = reinterpret_cast<const Fq*>(c->h_spark);
  const int cnts[3] = {6, 15, 2};
  const vpin::fq* tabs[3] = {S.derefs, comb_ops->d, comb_mem->d};
  const vpin::fq* eqs[3] = {eq_ops->d, eq_ops->d, eq_mem->d};
  Fq mine23[23] = {}, all23[23];
  int rc, base = 0;
  if (S.st) {
    // every rank evaluates its residue class of all 23 slices; the partial sums (scaled by eq(rand_lo, rank)) are added up
    const size_t rk = S.leaves.r0, Wz = S.leaves.step;
    std::vector<Fq> lo_ops(Wz), lo_mem(Wz);
    host_eq(S.rand_ops.data() + (S.lgN - dz->lw), (size_t)dz->lw, lo_ops.data());
    host_eq(S.rand_mem.data() + (S.lgM - dz->lw), (size_t)dz->lw, lo_mem.data());
    const Fq scale[3] = {lo_ops[rk], lo_ops[rk], lo_mem[rk]};
    for (int g = 0; g < 3; g++) {
      // the derefs slices are this rank's local view already; the combined polynomials are whole
      if (g == 0) rc = vpin::spark_slice_evals(c, tabs[g], S.Nf, cnts[g], eqs[g]);
      else rc = vpin::spark_slice_evals(c, tabs[g], g == 1 ? N : M, cnts[g], eqs[g], rk, Wz);
      if (rc) return rc;
      for (int i = 0; i < cnts[g]; i++) mine23[base + i] = hs[3 * i] * scale[g];
      base += cnts[g];
    }
    if ((rc = dist_sum(c, *dz, mine23, 23, all23, "hash_slice_evals"))) return rc;
  } else {
    // deal them out in contiguous runs of equal cost (a slice costs its length), evaluate, exchange 23 scalars
    const size_t cost[3] = {N, N, M};
    size_t total = 0, cum = 0;
    for (int g = 0; g < 3; g++) total += cost[g] * (size_t)cnts[g];
    int owner[23];
    for (int g = 0, sidx = 0; g < 3; g++)
      for (int i = 0; i < cnts[g]; i++, sidx++) {
        owner[sidx] = (int)std::min<size_t>((size_t)dz->world - 1, (cum + cost[g] / 2) * (size_t)dz->world / total);
        cum += cost[g];
      }
    for (int g = 0; g < 3; g++) {
      int first = -1, cnt = 0;
      for (int i = 0; i < cnts[g]; i++)
        if (owner[base + i] == dz->rank) { if (first < 0) first = i; cnt++; }
      if (cnt) {  // a rank's slices of one table are contiguous
        if ((rc = vpin::spark_slice_evals(c, tabs[g] + (size_t)first * cost[g], cost[g], cnt, eqs[g]))) return rc;
        for (int i = 0; i < cnt; i++) mine23[base + first + i] = hs[3 * i];
      }
      base += cnts[g];
    }
    if ((rc = dist_pick(c, *dz, mine23, 23, owner, all23, "hash_slice_evals"))) return rc;
  }
  std::copy(all23, all23 + 6, S.ev_derefs);
  std::copy(all23 + 6, all23 + 21, S.ev_ops);
  std::copy(all23 + 21, all23 + 23, S.ev_mem);
  return VPIN_OK;
}

// the joint evaluation proof of one combined polynomial Z (DerefsEvalProof::prove :137-158, :90-135; HashLayerProof::prove
// :803-849): its slices' evaluations e (padded to a power of two) at `rand`, combined with nch challenges
struct JointLabels { const char *evals, *challenge, *joint, *span; };
static int prove_joint(SparkProof& S, const PcGens& g, const vpin_table* Z, SlicePass& sp, const std::vector<Fq>& e, int nch,
                       const std::vector<Fq>& rand, const JointLabels& lab, const vpin::fq* z_rows, DpLog& out) {
  int rc;
  S.tr.append_scalars(lab.evals, e.data(), e.size());
  std::vector<Fq> ch = S.tr.challenge_vector(lab.challenge, nch);
  Fq joint = combine_bot(e, ch);
  std::vector<Fq> rj(ch);
  rj.insert(rj.end(), rand.begin(), rand.end());
  S.tr.append_scalar(lab.joint, joint);
  TraceSpan ts(lab.span);
  std::vector<Fq> lz;
  if (sp.on && (rc = sp.combine(S.c, g, ch, lz))) return rc;
  if ((rc = polyeval_prove_plain(S.c, g, Z, rj, joint, S.tr, S.tape, out, z_rows, sp.on ? &lz : nullptr, sp.on ? &sp.Rv : nullptr))) return rc;
  return vpin::comm_mark(S.c, "hash_bullet");
}

// HashLayerProof::prove (:740-849)
static int stage_hash(SparkProof& S) {
  vpin_ctx* c = S.c;
  const vpin_spark_decomm* d = S.d;
  const DistPlan* dz = S.dz;
  const size_t N = S.N, M = S.M;
  const std::vector<Fq>&rand_ops = S.rand_ops, &rand_mem = S.rand_mem;
  int rc;
  S.tr.append_protocol_name("Sparse polynomial hash layer proof");
  vpin_table *eq_ops = nullptr, *eq_mem = nullptr;
  // single GPU: slice evaluations and the evaluation proofs' LZ vectors from one pass per combined polynomial (SlicePass)
  const bool one_pass = !dz && SlicePass::fits(*S.g_derefs, 3, rand_ops) && SlicePass::fits(*S.g_ops, 4, rand_ops) &&
                        SlicePass::fits(*S.g_mem, 1, rand_mem);
  SlicePass sp_derefs(c), sp_ops(c), sp_mem(c);
  // the combined polynomials as whole field tables: only the two-pass and the multi-GPU paths read them (this proof's own
  // copies: the decommitment is shared with other contexts)
  vpin_table *comb_ops = nullptr, *comb_mem = nullptr;
  if (!one_pass && dz) {
    // a proof split over several GPUs: built once per decommitment on first use and kept (the ranks of a rehearsal share one
    // decommitment and one copy; on a real node every GPU holds its own)
    auto* dm = const_cast<vpin_spark_decomm*>(d);
    dm->comb_unpooled = true;
    if ((rc = vpin::spark_comb_tables(c, dm))) return rc;
    comb_ops = dm->comb_ops; comb_mem = dm->comb_mem;
  } else if (!one_pass) {
    if ((rc = vpin::spark_comb_make(c, d, &comb_ops, &comb_mem))) return rc;
    S.tg.add(comb_ops); S.tg.add(comb_mem);
  }
  if (!one_pass) {
    TraceSpan ts("hash: eq tables");
    // split by residue class: eq(rand, rank + k W) = eq(rand_hi, k) * eq(rand_lo, rank), so the local table is the table of
    // the first lg - lw challenges and the rank's sums are scaled by one constant
    const int lwz = S.st ? dz->lw : 0;
    if ((rc = vpin_eq_table(c, B(rand_ops.data()), (int)S.lgN - lwz, &eq_ops))) return rc;
    S.tg.add(eq_ops);
    if ((rc = vpin_eq_table(c, B(rand_mem.data()), (int)S.lgM - lwz, &eq_mem))) return rc;
    S.tg.add(eq_mem);
  }
  if ((rc = vpin::comm_mark(c, "hash_eq_tables"))) return rc;
  const Fq* hs = reinterpret_cast<const Fq*>(c->h_spark);
  if (dz) {
    if ((rc = hash_slice_evals_dist(S, comb_ops, comb_mem, eq_ops, eq_mem))) return rc;
  } else if (one_pass) {
    TraceSpan ts("hash: derefs slices (one pass)");
    if ((rc = sp_derefs.run(c, *S.g_derefs, nullptr, 0, S.derefs, 3, 6, rand_ops, S.ev_derefs))) return rc;
  } else {
    TraceSpan ts("hash: derefs slice evals");
    if ((rc = vpin::spark_slice_evals(c, S.derefs, N, 6, eq_ops->d))) return rc;
    for (int i = 0; i < 6; i++) S.ev_derefs[i] = hs[3 * i];
  }
  S.tr.append_protocol_name("Derefs evaluation proof");
  std::vector<Fq> e8(8, Fq::zero());
  std::copy(S.ev_derefs, S.ev_derefs + 6, e8.begin());
  if ((rc = prove_joint(S, *S.g_derefs, S.comb, sp_derefs, e8, 3, rand_ops,
                        {"evals_ops_val", "challenge_combine_n_to_one", "joint_claim_eval", "hash: polyeval derefs"}, S.comb_rows, S.pe_derefs)))
    return rc;
  if (one_pass) {
    TraceSpan ts("hash: ops+mem slices (one pass)");
    if ((rc = sp_ops.run(c, *S.g_ops, d->idx, 12, d->vals, 4, 15, rand_ops, S.ev_ops))) return rc;
    if ((rc = sp_mem.run(c, *S.g_mem, d->idx + 12 * N, 2, nullptr, 1, 2, rand_mem, S.ev_mem))) return rc;
  } else if (!dz) {
    TraceSpan ts("hash: ops+mem slice evals");
    if ((rc = vpin::spark_slice_evals(c, comb_ops->d, N, 15, eq_ops->d))) return rc;
    for (int i = 0; i < 15; i++) S.ev_ops[i] = hs[3 * i];
    if ((rc = vpin::spark_slice_evals(c, comb_mem->d, M, 2, eq_mem->d))) return rc;
    for (int i = 0; i < 2; i++) S.ev_mem[i] = hs[3 * i];
  }
  std::vector<Fq> e16(16, Fq::zero());
  std::copy(S.ev_ops, S.ev_ops + 15, e16.begin());  // row addr, row read_ts, col addr, col read_ts, val (comb_ops order)
  if ((rc = prove_joint(S, *S.g_ops, comb_ops, sp_ops, e16, 4, rand_ops,
                        {"claim_evals_ops", "challenge_combine_n_to_one", "joint_claim_eval_ops", "hash: polyeval ops"}, nullptr, S.pe_ops)))
    return rc;
  return prove_joint(S, *S.g_mem, comb_mem, sp_mem, {S.ev_mem[0], S.ev_mem[1]}, 1, rand_mem,
                     {"claim_evals_mem", "challenge_combine_two_to_one", "joint_claim_eval_mem", "hash: polyeval mem"}, nullptr, S.pe_mem);
}

// bincode(R1CSEvalProof) (r1csinstance.rs:326-328; sparse_mlpoly.rs:1438-1441,1326-1329,1036-1042,698-707)
static void write_proof(const SparkProof& S, Writer& w) {
  const auto& pl = S.pl;
  w.u64(S.comm_derefs.size());
  for (auto& p : S.comm_derefs) w.point(p);
  for (int s = 0; s < 2; s++) { w.scalar(pl[s][0]); w_scalars(w, &pl[s][1], 3); w_scalars(w, &pl[s][4], 3); w.scalar(pl[s][7]); }
  w_scalars(w, S.dotp_left, 3);
  w_scalars(w, S.dotp_right, 3);
  write_batched(w, S.pf_mem);
  write_batched(w, S.pf_ops);
  w_scalars(w, &S.ev_ops[0], 3); w_scalars(w, &S.ev_ops[3], 3); w.scalar(S.ev_mem[0]);  // eval_row: addr, read_ts, audit_ts
  w_scalars(w, &S.ev_ops[6], 3); w_scalars(w, &S.ev_ops[9], 3); w.scalar(S.ev_mem[1]);  // eval_col
  w_scalars(w, &S.ev_ops[12], 3);                                                       // eval_val
  w_scalars(w, &S.ev_derefs[0], 3); w_scalars(w, &S.ev_derefs[3], 3);                   // eval_derefs
  write_dplog(w, S.pe_ops);
  write_dplog(w, S.pe_mem);
  write_dplog(w, S.pe_derefs);
}

// SparseMatPolyEvalProof::prove (sparse_mlpoly.rs:1466-1533) -> bincode(R1CSEvalProof) appended to w
// spark_begin: the shapes, the generator views and the split; spark_finish: the stages and the proof's bytes.  A whole SNARK on
// one GPU calls spark_inst_evals between the two, from inside its sat proof.
static int spark_begin(SparkProof& S) {
  vpin_ctx* c = S.c;
  const vpin_spark_decomm* d = S.d;
  if (d->N < 4 || d->M < 4 || S.rx.size() != d->nx || S.ry.size() != d->ny) return VPIN_ESHAPE;
  int rc;
  const Shape sh{d->nx, d->ny, S.N, S.M, S.lgN + 4, std::max(d->nx, d->ny) + 1, S.lgN + 3};
  // the longest stream first: a later, longer request would rebuild the table and drop earlier views
  if ((rc = get_view(c, std::max(sh.v_ops, sh.v_mem), &S.g_ops)) || (rc = get_view(c, sh.v_ops, &S.g_ops)) ||
      (rc = get_view(c, sh.v_mem, &S.g_mem)) || (rc = get_view(c, sh.v_derefs, &S.g_derefs)))
    return rc;
  return split_plan(S);
}

// inst.evaluate(rx, ry) = (A, B, C)(rx, ry) from the SPARK prover's own first pass: M(rx, ry) = sum_k val_k eq(rx, row_k)
// eq(ry, col_k) is the sum of the matrix's two dot-product halves over the derefs polynomial.  The tables and the six sums stay in
// S for stage_derefs and dotp_claims (which still checks left + right against these evaluations).
static int spark_inst_evals(SparkProof& S, Fq ie[3]) {
  vpin_ctx* c = S.c;
  int rc;
  if (S.dz) return VPIN_EINVAL;  // one GPU only: a split proof sums per rank, after its gather
  if ((rc = derefs_tables(S))) return rc;
  if ((rc = vpin::spark_triple_sums(c, S.derefs, S.vals, S.Nf, nullptr, 6))) return rc;
  for (int i = 0; i < 6; i++) S.sums6[i] = reinterpret_cast<const Fq*>(c->h_spark)[3 * i];
  S.have_sums = true;
  for (int m = 0; m < 3; m++) ie[m] = S.sums6[2 * m] + S.sums6[2 * m + 1];
  return VPIN_OK;
}

static int spark_finish(SparkProof& S, Writer& w) {
  vpin_ctx* c = S.c;
  int rc;
  // one stage per timing slot of vpin_spark_last_timings
  auto t0 = Clock::now();
  auto lap = [&](int slot) { g_spark_timings[slot] = secs(t0, Clock::now()); t0 = Clock::now(); };
  if ((rc = stage_derefs(S))) return rc;
  lap(1);
  if (c->progress_flag) *c->progress_flag = 2;  // the proof's largest MSM is done (a scheduler may let other streams in now)
  if ((rc = stage_network(S))) return rc;
  lap(2);
  if ((rc = stage_product(S))) return rc;
  lap(3);
  if ((rc = stage_hash(S))) return rc;
  lap(4);
  write_proof(S, w);
  return VPIN_OK;
}

}  // namespace

extern "C" {

size_t vpin_spark_comm_bytes(const vpin_r1cs* inst) {
  return inst ? vpin_sizes::spark_comm_bytes(inst->num_cons, inst->num_vars, inst->nnz) : 0;
}

size_t vpin_snark_proof_max_bytes(const vpin_r1cs* inst) {
  return inst ? vpin_sizes::snark_proof_max_bytes(inst->num_cons, inst->num_vars, inst->nnz) : 0;
}

int vpin_spark_prepare(vpin_ctx* c, size_t num_cons, size_t num_vars, size_t max_nnz) {
  if (!c || !vpin::is_pow2(num_cons) || !vpin::is_pow2(num_vars) || max_nnz == 0) return VPIN_EINVAL;
  (void)hipSetDevice(c->device);
  const size_t nnz[3] = {max_nnz, max_nnz, max_nnz};
  const Shape s = shape_of(num_cons, num_vars, nnz);
  const PcGens* g = nullptr;
  int rc = get_view(c, std::max(s.v_ops, s.v_mem), &g);
  if (!rc) {
    // the host fixed-base tables of the other views' two blind generators (~3 ms each, kept per process and point): all at once
    auto* sg = static_cast<SparkGens*>(c->spark_cache);
    std::vector<size_t> idx;
    for (size_t ell : {s.v_ops, s.v_mem, s.v_derefs}) {
      const size_t R = (size_t)1 << (ell - ell / 2);
      if (R + 1 < sg->g.size()) { idx.push_back(R); idx.push_back(R + 1); }
    }
#pragma omp parallel for schedule(dynamic, 1) num_threads(host_threads())
    for (long k = 0; k < (long)idx.size(); k++) { FixedBase warm(sg->g[idx[(size_t)k]]); (void)warm; }
  }
  if (!rc) rc = get_view(c, s.v_ops, &g);
  if (!rc) rc = get_view(c, s.v_mem, &g);
  if (!rc) rc = get_view(c, s.v_derefs, &g);
  return rc;
}

int vpin_spark_gens_view(vpin_ctx* c, size_t ell, const vpin_gens** out, size_t* L, size_t* R) {
  if (!c || !out || !L || !R || ell < 2 || ell > 40) return VPIN_EINVAL;
  (void)hipSetDevice(c->device);
  const PcGens* g = nullptr;
  int rc = get_view(c, ell, &g);
  if (rc) return rc;
  *out = g->dev; *L = g->L; *R = g->R;
  return VPIN_OK;
}

int vpin_dist_plan(int world, int owner_ops[12], int owner_dotp[6], int owner_mem[4]) {
  if (world < 1 || world > 12 || !owner_ops || !owner_dotp || !owner_mem) return VPIN_EINVAL;
  make_plan(world, owner_ops, owner_dotp, owner_mem);
  return VPIN_OK;
}

void vpin_spark_decomm_hot_cols(const vpin_spark_decomm* d, uint32_t out[3]) {
  for (int m = 0; m < 3; m++) out[m] = d ? d->hot_col[m] : 0xffffffffu;
}

void vpin_spark_decomm_free(vpin_ctx* c, vpin_spark_decomm* d) {
  if (!d) return;
  if (c) {
    (void)hipSetDevice(c->device);
    if (d->idx) vpin::dev_free(c, d->idx);
    if (d->vals) vpin::dev_free(c, d->vals);
    if (d->comb_ops) vpin_table_free(c, d->comb_ops);
    if (d->comb_mem) vpin_table_free(c, d->comb_mem);
  }
  delete d;
}

// second half of SNARK::encode: commit comb_ops / comb_mem (dense_mlpoly.rs:193-218 under b"gens_r1cs_eval") and
// serialise bincode(R1CSCommitment) (r1csinstance.rs:53-58, sparse_mlpoly.rs:332-338)
static int encode_commit(vpin_ctx* c, const Shape& s, std::unique_ptr<vpin_spark_decomm>& d, vpin::TraceLap& lap, size_t num_cons,
                         size_t num_vars, size_t num_inputs, vpin_spark_decomm** out, uint8_t* comm_out, size_t comm_cap,
                         size_t* comm_len, Clock::time_point t0) {
  auto fail = [&](int rc) { vpin_spark_decomm_free(c, d.release()); return rc; };
  int rc;
  const PcGens *g_ops = nullptr, *g_mem = nullptr;
  if ((rc = get_view(c, std::max(s.v_ops, s.v_mem), &g_ops)) || (rc = get_view(c, s.v_ops, &g_ops)) ||
      (rc = get_view(c, s.v_mem, &g_mem)))
    return fail(rc);
  lap("generators (views)");
  std::vector<CG> c_ops, c_mem;
  if ((rc = vpin::spark_comb_tables(c, d.get()))) return fail(rc);
  lap("comb tables");
  // 13 of comb_ops' 16 slices and all of comb_mem are addresses, timestamps and counters
  if ((rc = commit_noblind(c, g_ops, d->comb_ops, c_ops, true))) return fail(rc);
  lap("commit ops");
  if ((rc = commit_noblind(c, g_mem, d->comb_mem, c_mem, true))) return fail(rc);
  lap("commit mem");
  // (commit_noblind has synchronised the stream.)  The blocks go back to the context's POOL, never straight to the driver
  // (round 6): the proof that follows takes its 16N-scalar temporaries out of them, and a host that encodes per proof
  // (vpin_snark_prove from host buffers) would otherwise pay a 17 GB hipMalloc / hipFree pair every time -- 0.3 ms usually,
  // seconds every few calls (bench.py --trace E --host-buffers: 106 -> 975 ms/step when it struck).  A service that encodes
  // once and keeps proving trims the pool after its set-up (vpin_ctx_pool_trim), as bench.py does.
  vpin::spark_comb_release(c, d.get(), false);
  lap("comb release");
  if ((rc = vpin::spark_find_hot_cols(c, d.get()))) return fail(rc);
  lap("hot columns");
  Writer w;
  w.u64(num_cons); w.u64(num_vars); w.u64(num_inputs);
  w.u64(3); w.u64(s.N); w.u64(s.M);
  w.u64(c_ops.size()); for (auto& p : c_ops) w.point(p);
  w.u64(c_mem.size()); for (auto& p : c_mem) w.point(p);
  if (w.buf.size() > comm_cap) return fail(VPIN_ESHAPE);
  memcpy(comm_out, w.buf.data(), w.buf.size());
  *comm_len = w.buf.size();
  *out = d.release();
  g_spark_timings[0] = secs(t0, Clock::now());
  return VPIN_OK;
}

// SNARK::encode (lib.rs:347-359) = R1CSInstance::commit (r1csinstance.rs:309-322) =
// SparseMatPolynomial::multi_commit (sparse_mlpoly.rs:500-520)
int vpin_spark_encode(vpin_ctx* c, const vpin_r1cs* inst, vpin_spark_decomm** out, uint8_t* comm_out, size_t comm_cap,
                      size_t* comm_len) {
  if (!c || !inst || !out || !comm_out || !comm_len) return VPIN_EINVAL;
  if (!vpin::is_pow2(inst->num_cons) || !vpin::is_pow2(inst->num_vars) || inst->num_inputs >= inst->num_vars) return VPIN_ESHAPE;
  auto t0 = Clock::now();
  (void)hipSetDevice(c->device);
  const Shape s = shape_of(inst->num_cons, inst->num_vars, inst->nnz);
  const size_t N = s.N, M = s.M;
  if (N < 4 || M < 4 || M > ((size_t)1 << 32) || N > ((size_t)1 << 31)) return VPIN_ESHAPE;
  if (comm_cap < vpin_spark_comm_bytes(inst)) return VPIN_ESHAPE;
  for (int m = 0; m < 3; m++)
    if (inst->nnz[m] && (!inst->row[m] || !inst->col[m] || !inst->val[m])) return VPIN_EINVAL;
  std::unique_ptr<vpin_spark_decomm> d(new vpin_spark_decomm());
  d->num_cons = inst->num_cons; d->num_vars = inst->num_vars; d->num_inputs = inst->num_inputs;
  d->nx = s.nx; d->ny = s.ny; d->N = N; d->M = M;
  auto fail = [&](int rc) { vpin_spark_decomm_free(c, d.release()); return rc; };

  // sparse_to_dense_vecs (:368-380) + AddrTimestamps::new (:232-265).  Round 5: on the device -- the addresses go up as they
  // are (padded entries read address 0), the time stamps come from a stable sort of each side's 3N accesses (trace.hip); the
  // host used to walk both traces sequentially (60 % of this call for CNN A).
  vpin::TraceLap lap(c, "spark_encode");
  int rc;
  if ((rc = vpin::dev_alloc(c, (12 * N + 2 * M) * 4, (void**)&d->idx))) return fail(rc);
  vpin::DevBuf b_bad(c);
  if (b_bad.alloc(4)) return fail(VPIN_ENOMEM);
  if (hipMemsetAsync(b_bad.p, 0, 4, c->stream) != hipSuccess) return fail(VPIN_EHIP);
  for (int side = 0; side < 2; side++) {
    uint32_t* addr = d->idx + (size_t)side * 6 * N;
    if (hipMemsetAsync(addr, 0, 3 * N * 4, c->stream) != hipSuccess) return fail(VPIN_EHIP);
    for (int m = 0; m < 3; m++) {
      const uint32_t* src = side ? inst->col[m] : inst->row[m];
      if (inst->nnz[m] && hipMemcpyAsync(addr + (size_t)m * N, src, inst->nnz[m] * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return fail(VPIN_EHIP);
      if ((rc = vpin::spark_check_bounds(c, addr + (size_t)m * N, inst->nnz[m], (uint32_t)(side ? 2 * inst->num_vars : inst->num_cons),
                                         (uint32_t*)b_bad.p)))
        return fail(rc);
    }
    if ((rc = vpin::spark_trace_timestamps(c, addr, 3 * N, M, addr + 3 * N, d->idx + 12 * N + (size_t)side * M))) return fail(rc);
  }
  uint32_t bad = 0;
  if (hipMemcpyAsync(&bad, b_bad.p, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
    return fail(VPIN_EHIP);
  if (bad) return fail(VPIN_ESHAPE);  // lib.rs:171-178 InvalidIndex
  b_bad.release();
  lap("device idx + timestamps");
  if ((rc = vpin::dev_alloc(c, 3 * N * 32, (void**)&d->vals))) return fail(rc);
  if (hipMemsetAsync(d->vals, 0, 3 * N * 32, c->stream) != hipSuccess) return fail(VPIN_EHIP);
  for (int m = 0; m < 3; m++)
    if (inst->nnz[m] && hipMemcpyAsync(d->vals + (size_t)m * N, inst->val[m], inst->nnz[m] * 32, hipMemcpyHostToDevice,
                                       c->stream) != hipSuccess)
      return fail(VPIN_EHIP);
  if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(VPIN_EHIP);
  lap("upload + comb tables");

  return encode_commit(c, s, d, lap, inst->num_cons, inst->num_vars, inst->num_inputs, out, comm_out, comm_cap, comm_len, t0);
}

// SNARK::encode for a device-built gadget instance: the dense representation comes from gadget_dev.hip's
// closed forms instead of the host's sequential memory trace
int vpin_spark_encode_dev(vpin_ctx* c, const vpin_dev_instance* g, vpin_spark_decomm** out, uint8_t* comm_out, size_t comm_cap,
                          size_t* comm_len) {
  if (!c || !g || !g->r1cs || !out || !comm_out || !comm_len) return VPIN_EINVAL;
  auto t0 = Clock::now();
  (void)hipSetDevice(c->device);
  const size_t num_cons = g->r1cs->num_cons, num_vars = g->r1cs->num_vars;
  const Shape s = shape_of(num_cons, num_vars, g->nnz);
  const size_t N = s.N, M = s.M;
  if (N < 4 || M < 4 || M > ((size_t)1 << 32) || N > ((size_t)1 << 31)) return VPIN_ESHAPE;
  if (comm_cap < vpin_dev_instance_comm_bytes(g)) return VPIN_ESHAPE;
  std::unique_ptr<vpin_spark_decomm> d(new vpin_spark_decomm());
  d->num_cons = num_cons; d->num_vars = num_vars; d->num_inputs = g->num_inputs;
  d->nx = s.nx; d->ny = s.ny; d->N = N; d->M = M;
  auto fail = [&](int rc) { vpin_spark_decomm_free(c, d.release()); return rc; };
  vpin::TraceLap lap(c, "spark_encode_dev");
  int rc;
  if ((rc = vpin::dev_alloc(c, (12 * N + 2 * M) * 4, (void**)&d->idx))) return fail(rc);
  if ((rc = vpin::dev_alloc(c, 3 * N * 32, (void**)&d->vals))) return fail(rc);
  if ((rc = vpin::gadget_fill_decomm(c, g, d.get()))) return fail(rc);
  lap("trace + comb tables");
  return encode_commit(c, s, d, lap, num_cons, num_vars, g->num_inputs, out, comm_out, comm_cap, comm_len, t0);
}

size_t vpin_dev_instance_comm_bytes(const vpin_dev_instance* g) {
  if (!g || !g->r1cs) return 0;
  vpin_r1cs r{};
  r.num_cons = g->r1cs->num_cons; r.num_vars = g->r1cs->num_vars; r.num_inputs = g->num_inputs;
  for (int m = 0; m < 3; m++) r.nnz[m] = g->nnz[m];
  return vpin_spark_comm_bytes(&r);
}

size_t vpin_dev_instance_proof_max_bytes(const vpin_dev_instance* g) {
  if (!g || !g->r1cs) return 0;
  vpin_r1cs r{};
  r.num_cons = g->r1cs->num_cons; r.num_vars = g->r1cs->num_vars; r.num_inputs = g->num_inputs;
  for (int m = 0; m < 3; m++) r.nnz[m] = g->nnz[m];
  return vpin_snark_proof_max_bytes(&r);
}

// Kernel-level entry of the hash layer's one-pass slice evaluation (include/vpin_hip.h)
int vpin_poly_slices_bound(vpin_ctx* c, const vpin_table* Z, int nbits, int used, const uint8_t* r, size_t r_len, const uint8_t* ch,
                           uint8_t* evals_out, uint8_t* LZ_out) {
  if (!c || !Z || !Z->d || nbits < 0 || nbits > 4 || used < 1 || used > (1 << nbits) || !r || !evals_out) return VPIN_EINVAL;
  const size_t ell = r_len + (size_t)nbits;
  if (Z->len != ((size_t)1 << ell) || ell / 2 < (size_t)nbits) return VPIN_ESHAPE;
  PcGens pc;  // shape only
  pc.ell = ell; pc.L = (size_t)1 << (ell / 2); pc.R = (size_t)1 << (ell - ell / 2);
  std::vector<Fq> rand(r_len);
  memcpy(rand.data(), r, r_len * 32);
  SlicePass sp(c);
  std::vector<Fq> ev((size_t)used);
  int rc = sp.run(c, pc, nullptr, 0, Z->d, nbits, used, rand, ev.data());
  if (rc) return rc;
  memcpy(evals_out, ev.data(), (size_t)used * 32);
  if (ch && LZ_out) {
    std::vector<Fq> chv((size_t)nbits), LZ;
    memcpy(chv.data(), ch, (size_t)nbits * 32);
    if ((rc = sp.combine(c, pc, chv, LZ))) return rc;
    memcpy(LZ_out, LZ.data(), pc.R * 32);
  }
  return VPIN_OK;
}

// the same with the first n32 slices given as u32 (host memory, n32 x N values: the decommitment's addresses and timestamps,
// whose field images Scalar::from(v) are never formed) and the other used - n32 slices as a table of field elements
int vpin_poly_slices_bound_u32(vpin_ctx* c, const uint32_t* slices_u32, int n32, const vpin_table* Zfq, int nbits, int used,
                               const uint8_t* r, size_t r_len, const uint8_t* ch, uint8_t* evals_out, uint8_t* LZ_out) {
  if (!c || !slices_u32 || n32 < 1 || nbits < 0 || nbits > 4 || used < n32 || used > (1 << nbits) || !r || !evals_out) return VPIN_EINVAL;
  const size_t ell = r_len + (size_t)nbits, N = (size_t)1 << r_len;
  if (ell / 2 < (size_t)nbits || (used > n32 && (!Zfq || !Zfq->d || Zfq->len < (size_t)(used - n32) * N))) return VPIN_ESHAPE;
  PcGens pc;  // shape only
  pc.ell = ell; pc.L = (size_t)1 << (ell / 2); pc.R = (size_t)1 << (ell - ell / 2);
  (void)hipSetDevice(c->device);
  vpin::DevBuf b32(c);
  if (b32.alloc((size_t)n32 * N * 4)) return VPIN_ENOMEM;
  if (hipMemcpyAsync(b32.p, slices_u32, (size_t)n32 * N * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) return VPIN_EHIP;
  std::vector<Fq> rand(r_len);
  memcpy(rand.data(), r, r_len * 32);
  SlicePass sp(c);
  std::vector<Fq> ev((size_t)used);
  int rc = sp.run(c, pc, (const uint32_t*)b32.p, n32, used > n32 ? Zfq->d : nullptr, nbits, used, rand, ev.data());
  if (rc) return rc;
  memcpy(evals_out, ev.data(), (size_t)used * 32);
  if (ch && LZ_out) {
    std::vector<Fq> chv((size_t)nbits), LZ;
    memcpy(chv.data(), ch, (size_t)nbits * 32);
    if ((rc = sp.combine(c, pc, chv, LZ))) return rc;
    memcpy(LZ_out, LZ.data(), pc.R * 32);
  }
  return VPIN_OK;
}

// my_lib_prove (commit_test.rs:59-133) in full: R1CSProof, inst_evals, R1CSEvalProof -> bincode(SNARK)
int vpin_snark_prove_resident(vpin_ctx* c, const vpin_r1cs_dev* dinst, const vpin_spark_decomm* decomm,
                              const vpin_table* vars_para, const vpin_table* vars_input, const vpin_table* vars,
                              const uint8_t* inputs, const uint8_t seed_commit64[64], const uint8_t seed_proof64[64],
                              uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* comm_para_out,
                              uint8_t* comm_input_out) {
  if (!c || !dinst || !decomm || !vars_para || !vars_input || !vars || !seed_commit64 || !seed_proof64 || !proof_out ||
      !proof_len || !comm_para_out || !comm_input_out)
    return VPIN_EINVAL;
  size_t nv, ncons, ni;
  vpin_r1cs_dims(dinst, &ncons, &nv, &ni);
  if (vars_para->len != nv || vars_input->len != nv || vars->len != nv || (ni && !inputs)) return VPIN_ESHAPE;
  if (decomm->num_cons != ncons || decomm->num_vars != nv || decomm->num_inputs != ni) return VPIN_ESHAPE;
  auto t0 = Clock::now();
  vpin::AltStreamGuard alt_guard(c);  // vpin_ctx_set_cumask_after_phase1: back on the first stream however this returns
  Transcript tr("snark_example"), tape("snark_example");
  uint8_t ie[96];
  std::vector<Fq> rx(log2z(ncons)), ry(log2z(2 * nv));
  size_t sat_len = 0;
  Fq evals[3];
  // One GPU: the sat proof takes inst.evaluate(rx, ry) from the SPARK prover's derefs pass (spark_inst_evals) instead of three
  // gather passes of its own over the matrices.  A proof split over several GPUs keeps vpin_r1cs_evaluate.
  const bool fused = !(c->comm && c->comm->world > 1);
  SparkProof S(c, decomm, rx, ry, evals, tr, tape);
  const vpin_prover::InstEvalsFn from_derefs = [&](const Fq* rx_, size_t nrx, const Fq* ry_, size_t nry, Fq out[3]) -> int {
    if (nrx != rx.size() || nry != ry.size()) return VPIN_ESHAPE;
    std::copy(rx_, rx_ + nrx, rx.begin());
    std::copy(ry_, ry_ + nry, ry.begin());
    int rc_ = spark_begin(S);
    return rc_ ? rc_ : spark_inst_evals(S, out);
  };
  // collective over c->comm: a failure of this rank alone (memory, a HIP error) fails the peers' next wait (comm_leave)
  int rc = sat_prove_core(c, dinst, nv, ncons, ni, vars_para, vars_input, vars, inputs, seed_commit64, seed_proof64, proof_out,
                          proof_cap, &sat_len, comm_para_out, comm_input_out, ie, B(rx.data()), B(ry.data()), &tr, &tape,
                          fused ? &from_derefs : nullptr);
  if (rc) return vpin::comm_leave(c->comm, rc);
  if (c->progress_flag) *c->progress_flag = 1;
  g_spark_timings[5] = secs(t0, Clock::now());
  Writer w;
  w.bytes(ie, 96);  // SNARK.inst_evals (lib.rs:334-338)
  memcpy(evals, ie, 96);
  if (!fused) rc = spark_begin(S);
  if (rc || (rc = spark_finish(S, w))) return vpin::comm_leave(c->comm, rc);
  if (sat_len + w.buf.size() > proof_cap) return VPIN_ESHAPE;
  memcpy(proof_out + sat_len, w.buf.data(), w.buf.size());
  *proof_len = sat_len + w.buf.size();
  g_spark_timings[6] = secs(t0, Clock::now());
  return VPIN_OK;
}

// proof_point_mult.rs:38-94 from host buffers: SNARK::encode, then my_lib_prove in full
int vpin_snark_prove(vpin_ctx* c, const vpin_r1cs* inst, const uint8_t* vars_para, const uint8_t* vars_input,
                     const uint8_t* vars, const uint8_t* inputs, const uint8_t seed_commit64[64], const uint8_t seed_proof64[64],
                     uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* comm_out, size_t comm_cap, size_t* comm_len,
                     uint8_t* comm_para_out, uint8_t* comm_input_out) {
  if (!c || !inst || !vars_para || !vars_input || !vars) return VPIN_EINVAL;
  const size_t nv = inst->num_vars;
  if (!vpin::is_pow2(nv) || !vpin::is_pow2(inst->num_cons) || inst->num_inputs >= nv) return VPIN_ESHAPE;
  vpin_r1cs_dev* dinst = nullptr;
  vpin_spark_decomm* decomm = nullptr;
  const bool trace = getenv("VPIN_CLI_TRACE") != nullptr;
  auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!trace) return;
    (void)hipStreamSynchronize(c->stream);
    auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[vpin_snark_prove] %-18s %9.1f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  };
  int rc = vpin_r1cs_upload(c, inst, &dinst);
  if (rc) return rc;
  lap("r1cs_upload");
  TableGuard tg(c);
  vpin_table *d_para = nullptr, *d_input = nullptr, *d_vars = nullptr;
  rc = vpin_spark_encode(c, inst, &decomm, comm_out, comm_cap, comm_len);
  lap("spark_encode");
  if (!rc) rc = vpin_table_upload(c, vars_para, nv, &d_para);
  if (!rc) { tg.add(d_para); rc = vpin_table_upload(c, vars_input, nv, &d_input); }
  if (!rc) { tg.add(d_input); rc = vpin_table_upload(c, vars, nv, &d_vars); }
  lap("witness_upload");
  if (!rc) {
    tg.add(d_vars);
    rc = vpin_snark_prove_resident(c, dinst, decomm, d_para, d_input, d_vars, inputs, seed_commit64, seed_proof64, proof_out,
                                   proof_cap, proof_len, comm_para_out, comm_input_out);
  }
  lap("prove_resident");
  vpin_spark_decomm_free(c, decomm);
  vpin_r1cs_free(c, dinst);
  return rc;
}

// the same span for a device-built instance (vpin_gadget_point_*_dev): nothing crosses PCIe but the proof
int vpin_snark_prove_dev(vpin_ctx* c, const vpin_dev_instance* g, const uint8_t seed_commit64[64], const uint8_t seed_proof64[64],
                         uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* comm_out, size_t comm_cap,
                         size_t* comm_len, uint8_t* comm_para_out, uint8_t* comm_input_out) {
  if (!c || !g || !g->r1cs) return VPIN_EINVAL;
  vpin_spark_decomm* decomm = nullptr;
  vpin::TraceLap lap(c, "vpin_snark_prove_dev");
  int rc = vpin_spark_encode_dev(c, g, &decomm, comm_out, comm_cap, comm_len);
  lap("spark_encode_dev");
  if (!rc)
    rc = vpin_snark_prove_resident(c, g->r1cs, decomm, g->vars_para, g->vars_input, g->vars, g->num_inputs ? g->inputs : nullptr,
                                   seed_commit64, seed_proof64, proof_out, proof_cap, proof_len, comm_para_out, comm_input_out);
  lap("prove_resident");
  vpin_spark_decomm_free(c, decomm);
  return rc;
}

// [0] encode, [1] derefs + commit, [2] network build, [3] product-layer proofs, [4] hash-layer proofs,
// [5] sat part, [6] whole prove
void vpin_spark_last_timings(double out[8]) { memcpy(out, g_spark_timings, sizeof g_spark_timings); }

}  // extern "C"
