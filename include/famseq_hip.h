/*
 * famseq_hip.h — C ABI of libfamseq_hip.so: the MI355X (gfx950) implementation of
 * FamSeq's `-method 1` Bayesian-network pedigree genotype posterior.
 *
 * Boundary being replaced (all cites into /root/reference/src):
 *   the per-site operator   bool family::calPostProbBN(bool Known,int chrType)  family.h:375,
 *                           family.cpp:750-1124 (CUDA twin family.cu:974-2305)
 *   fed by                  bool family::set_LK(const dMatrix<double>&)          family.h:344, family.cpp:698-748
 *   and drained by          get_postProb / get_postProbSingle / get_postRlt      family.h:262,265,308
 *   called from             file.cpp:595->607->680-682, :833->845->918-920, :1743->1751->1804-1806
 * The reference crosses host->device once per site (6 cudaMalloc + 5 H2D + 1 launch
 * + 1 D2H per site, family.cu:1152-1703).  This ABI re-cuts the same operator as a
 * BATCH of sites per call: plain pointers and sizes, no C++ or torch types.
 *
 * Data layout (both directions): [n_sites][n_members][3] fp64, row-major, members in
 * PED order, genotype order RR,RA,AA — i.e. dMatrix<double> N x 3 (dMatrix.h:141-151)
 * repeated per site.  flags[s]: bit0 = Known (ID != "."), bit1 = chrX (file.cpp:476-486).
 *
 * status[s] (replaces the bool return + flagPB/flagPBS, family.cpp:752-763, :946-949):
 *   0     ok, full enumeration
 *   0x80  ok, took the -LRC single-sample shortcut (family.cpp:767-878)
 *   1     calPostProbSingle failed: a lk*prior row sum <= 0 (family.cpp:1437); post and
 *         post_single are NaN-filled — the caller prints `:NA:NA:NA` (file.cpp:607-620)
 *   2     BN row sum <= 0 (family.cpp:946/:1111); post is NaN-filled, post_single valid
 *
 * There is NO CPU fallback: every compute entry point fails (negative return, message
 * in famseq_last_error) when no gfx950 device is usable.
 */
#ifndef FAMSEQ_HIP_H_
#define FAMSEQ_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Limit of the 3^N enumeration engines (and the size of famseq_model's arrays): the reference CUDA file's own,
 * geno[20], pTmp[60] (family.cu:771-772) — 3^20 = 3.5e9 configurations per site is past any use of an enumeration
 * anyway.  The sum-product engine (FAMSEQ_ENGINE_ELIM) has no member limit, like the reference's CPU code
 * (std::vector state, family.cpp:894-941; its -method 2 peeling, :1126-1403, :1501-1845): see famseq_pedigree. */
#define FAMSEQ_MAX_MEMBERS 20

#define FAMSEQ_ST_OK 0
#define FAMSEQ_ST_SINGLE_FAIL 1
#define FAMSEQ_ST_BN_FAIL 2
#define FAMSEQ_ST_SHORTCUT 0x80

#define FAMSEQ_FLAG_KNOWN 1
#define FAMSEQ_FLAG_CHRX 2

/* engines (famseq_set_option "engine") */
#define FAMSEQ_ENGINE_ENUM 0 /* 3^N joint-genotype enumeration: any pedigree (the reference's -method 1 algorithm) */
#define FAMSEQ_ENGINE_ELIM 1 /* exact sum-product on the pedigree's factor graph: same marginals in O(27 N) per
                                site (pedigrees with loops: conditioned on up to three members, x3 per member);
                                kernel generated and compiled per pedigree */

/* error codes (negative returns) */
#define FAMSEQ_E_ARG (-1)      /* bad argument / model rejected */
#define FAMSEQ_E_NODEVICE (-2) /* no usable gfx950 device, or ctx created without one */
#define FAMSEQ_E_HIP (-3)      /* HIP runtime error, see famseq_last_error */
#define FAMSEQ_E_PED_HALF (-10) /* member with exactly one known parent (family.cpp:319-323) */
#define FAMSEQ_E_PED_SEX (-11)  /* mother not female / father not male (family.cpp:204-219) */

/* Everything `family` holds after setFam()+init() that the path reads
 * (file.cpp:1888-1927; family.cpp:78-127, 221-238). */
typedef struct {
  int32_t n_members;                     /* numInd, 1..FAMSEQ_MAX_MEMBERS */
  int32_t mother[FAMSEQ_MAX_MEMBERS];    /* parent[i][0] or -1            family.cpp:329 */
  int32_t father[FAMSEQ_MAX_MEMBERS];    /* parent[i][1] or -1            family.cpp:330 */
  int32_t gender[FAMSEQ_MAX_MEMBERS];    /* 1 = male, anything else is treated as female (family.cpp:1054) */
  uint8_t sequenced[FAMSEQ_MAX_MEMBERS]; /* 1 if the member is in mapV2P (has a VCF/LK column); the
                                            shortcut vote runs over these only (family.cpp:768-771) */
  double pcp2[27];   /* autosome   [child*9 + mother*3 + father]  family.cpp:447-550 */
  double pcp2Xf[27]; /* chrX daughter                             family.cpp:383-416 */
  double pcp2Xm[27]; /* chrX son                                  family.cpp:418-445 */
  double genoProbN[3], genoProbK[3], genoProbXN[3], genoProbXK[3]; /* family.cpp:91-109 */
  double lc;         /* m_lc, -LRC                                family.cpp:253-257 */
} famseq_model;

/* The same for a pedigree of ANY size: the per-member arrays are the caller's ([n_members] each, copied by
 * famseq_create_pedigree; `sequenced` may be NULL = all sequenced).  Contexts of more than FAMSEQ_MAX_MEMBERS
 * members serve FAMSEQ_ENGINE_ELIM only — what the reference's -method 2 is recommended for ("family size > 7 and
 * loop-free", FamSeq_Manual.pdf p.1) — and answer FAMSEQ_E_ARG to a batch call while the engine is the enumeration. */
typedef struct {
  int32_t n_members;        /* numInd, >= 1 */
  const int32_t *mother;    /* [n_members] parent[i][0] or -1    family.cpp:329 */
  const int32_t *father;    /* [n_members] parent[i][1] or -1    family.cpp:330 */
  const int32_t *gender;    /* [n_members] 1 = male              family.cpp:1054 */
  const uint8_t *sequenced; /* [n_members] or NULL               family.cpp:768-771 */
  double pcp2[27], pcp2Xf[27], pcp2Xm[27];
  double genoProbN[3], genoProbK[3], genoProbXN[3], genoProbXK[3];
  double lc;
} famseq_pedigree;

typedef struct famseq_ctx famseq_ctx;

/* ---- one-time model setup (replaces family ctor + init()) ---------------- */

/* calPCP2S / calPCP2Xf / calPCP2Xm for mutation rate `mrate`, bit-faithful to the
 * reference's accumulation order.  Each output is 27 doubles. */
void famseq_transmission_tables(double mrate, double *pcp2, double *pcp2Xf, double *pcp2Xm);

/* PED columns -> model: default priors, tables for `mrate`, setRelation, checkPed.
 * `sequenced` may be NULL (all sequenced).  Returns 0 or FAMSEQ_E_*. */
int famseq_model_init(famseq_model *m, int32_t n_members, const int32_t *id, const int32_t *mother_id,
                      const int32_t *father_id, const int32_t *gender, const uint8_t *sequenced,
                      double mrate, double lc);

/* The same for famseq_pedigree: fills the priors, the tables and lc of *p, and the caller's mother_idx /
 * father_idx arrays ([n_members] each) with setRelation's indices, and points p->mother / p->father at them;
 * p->gender and p->sequenced point at the arguments (which must outlive p's use).  Returns 0 or FAMSEQ_E_*. */
int famseq_pedigree_init(famseq_pedigree *p, int32_t n_members, const int32_t *id, const int32_t *mother_id,
                         const int32_t *father_id, const int32_t *gender, const uint8_t *sequenced, double mrate,
                         double lc, int32_t *mother_idx, int32_t *father_idx);

/* ---- context -------------------------------------------------------------- */

int famseq_device_count(void); /* visible HIP devices; 0 when there is none */

/* Validates the model, builds the enumeration plan and (device_id >= 0) binds one GPU:
 * uploads constants, creates streams and staging buffers.  One ctx = one device = one
 * caller thread (multi-GPU = one process/ctx per device, sites sharded by the caller).
 * device_id < 0 builds a plan-only ctx (for inspection; compute calls return
 * FAMSEQ_E_NODEVICE).  On failure returns NULL with a message in err. */
famseq_ctx *famseq_create(const famseq_model *model, int device_id, char *err, size_t errlen);
/* ... from a size-independent model.  Up to FAMSEQ_MAX_MEMBERS members: exactly famseq_create.  Beyond: no
 * enumeration plan is built, the context starts on FAMSEQ_ENGINE_ELIM (generated and compiled here; fails with a
 * message when the pedigree's loops need more than three conditioned members). */
famseq_ctx *famseq_create_pedigree(const famseq_pedigree *pedigree, int device_id, char *err, size_t errlen);
void famseq_destroy(famseq_ctx *ctx);
const char *famseq_last_error(famseq_ctx *ctx);

/* Integer knobs; must be set before the first batch call.  Keys:
 *   "fixed_digits"  A: high members mapped onto lanes (team = 3^A lanes), 0..6
 *   "low_members"   L: childless members enumerated in the unrolled register loop, 1..5
 *   "block_threads" workgroup size (multiple of 64, <= 768)
 *   "grid_blocks"   persistent grid size (0 = auto: CUs x resident blocks)
 *   "chunk_sites"   host-staging chunk of famseq_bn_batch (0 = auto)
 *   "enum_impl"     which enumeration kernel serves FAMSEQ_ENGINE_ENUM: 0 = the team-per-site kernel
 *                   compiled into the library (any batch size, any pedigree, no compiler needed); 1 = the
 *                   kernel generated and compiled for this pedigree, one lane per site unless "group_digits"
 *                   says otherwise; -1 (default) = the generated kernel, lanes per site chosen by batch size,
 *                   for batches of >= "lane_min_sites" (256) sites when it can be built, the team kernel
 *                   otherwise (tiny calls never wait for a compile)
 *   "bulk_min_sites"  from how many sites on a one-lane-per-site launch of a context that is free to choose ("enum_impl" -1,
 *                   "group_digits" -1) is served by the large-batch form of the generated kernel (lane variants 8-11: the
 *                   super-leaf table built once per step of the outermost loop), where the pedigree has one; its posteriors
 *                   differ from the plain form's in their last bits.  Default: 16 chunks per resident wave (1,048,576 on
 *                   MI355X); -1 = never.  A host entry decides once per call, from the call's size; famseq_plan_json
 *                   "enum_last_kind" says which kernel served the last launch
 *   "tune"          1 = time the candidates of this pedigree's generated kernels on this device (where a static rule
 *                   picks a variant: the enumeration kernel's 7- or 6-member unrolled block, the sum-product kernel's
 *                   fence variant and where it keeps the likelihoods) on synthetic rows, a few milliseconds each, and keep the winners' indices as notes
 *                   in the kernel cache — every later context for the pedigree starts from them; compiles every
 *                   candidate (seconds each), needs a device; famseq_plan_json "tune" reports what was measured
 *   "pick_lane", "pick_elim"  a variant index measured elsewhere, kept as the note "tune" would leave (how build() ships
 *                   its table of measured picks); works on a plan-only context
 *   "prebuild_lane", "prebuild_elim"  compile that variant of the pedigree's kernel into the cache without loading it
 *                   (a plan-only context will do): how a build host prepares every candidate "tune" races
 *   "group_digits"  the generated kernel's lanes per site, 3^d: d = 0 one lane per site (large batches),
 *                   d = 1..4 lanes-per-site mode for batches too small to give every lane of the chip a
 *                   site (each lane of a group enumerates one combination of the d outermost looped
 *                   members' genotypes; the group sums through LDS); -1 (default) = chosen per call from
 *                   the batch size.  At most the number of looped members of the pedigree's enumeration
 *                   (famseq_plan_json "enum_group_digits_max"; 0 for pedigrees of up to 6 members)
 *   "phase_clock_report"  measuring aid: with FAMSEQ_PHASE_CLOCK=1 in the environment the generated kernels carry cycle marks between
 *                   their phases; this prints the plain kernels' shares (wave cycles per phase) on stderr and clears them
 *   "call_kernels"  1 = build the generated kernels' fused call-path forms now (famseq_bn_call_batch would on
 *                   its first call); 2 = only the form of the engine this ctx runs (what that first call loads)
 *   "engine"        FAMSEQ_ENGINE_ENUM (default) or FAMSEQ_ENGINE_ELIM; selecting ELIM generates the
 *                   kernel for this pedigree, compiles it (libhiprtc in-process; cached on disk) and fails with
 *                   FAMSEQ_E_ARG on a pedigree whose loops need more than three conditioned members
 * Returns 0 or FAMSEQ_E_ARG. */
int famseq_set_option(famseq_ctx *ctx, const char *key, int64_t value);

/* JSON description of the plan and launch geometry (valid until the next call on ctx). */
const char *famseq_plan_json(famseq_ctx *ctx);

/* ---- the operator ---------------------------------------------------------- */

/* Host buffers (pageable, or pinned for the full rate of the link).  Blocking.  Works in chunks
 * through three event-chained stages (copy in / compute / copy out, one HIP stream each) so that both
 * directions of the host link are busy at once.  post_single and status may be NULL.  Returns 0 or a
 * negative error.  (The host link bounds this entry point: 722 B/site at N = 10; see
 * famseq_bn_call_batch for the compact path.) */
int famseq_bn_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint8_t *flags,
                    double *post, double *post_single, uint8_t *status);

/* The same over several GPUs of one node from one process: ctxs[g] (one per device, created by the
 * caller for the same model) gets the contiguous site range [g*S/G, (g+1)*S/G) and its own host
 * thread; results land in the caller's arrays in site order.  No collective: sites are independent
 * (family.cpp:791 zeroes all state per site).  Returns 0, or the first error any
 * ctx reported (famseq_last_error on that ctx has the text). */
int famseq_bn_batch_sharded(famseq_ctx *const *ctxs, int n_ctx, int64_t n_sites, const double *lk, const uint8_t *flags,
                            double *post, double *post_single, uint8_t *status);

/* Device buffers already resident in HBM on ctx's device.  Enqueues on `stream`
 * (a hipStream_t; NULL = the default stream) and returns without synchronising.
 * d_post_single and d_status may be NULL.
 *
 * THE STREAM RULE, of this and of every other entry whose name ends in _device and that takes a stream (each refers here):
 *   - Everything the entry does on the device — kernels, and the small uploads some entries make — is enqueued on `stream`,
 *     in the order of the calls; the host returns while the stream may still be busy with what was put on it before.  The
 *     caller's buffers, inputs and outputs, belong to the call until the stream has passed it.
 *   - What may block the host is the first call of a kind or of a shape, and nothing after it: loading (or compiling) a
 *     kernel the context has not used yet, uploading a table on first use, and allocating or growing scratch this context
 *     keeps (famseq_bn_call_batch_device for batches that are not served fused or outputs the caller does not pass; the side
 *     entries' unpacked rows for d_pl16) — growing waits until every earlier call that uses that scratch has run, on
 *     whatever stream, and a batch no larger than one before it grows nothing.  Also: once 16 uploads of changed
 *     seq_members / changed pointers are enqueued and none has run, the next one waits for the oldest.
 *   - Calls that touch state the context keeps on the device — the column maps made from seq_members, the call path's
 *     argument block, the scratch above: famseq_bn_call_batch_device always, a side entry when it is given d_pl16 — take
 *     effect in the order they are issued, whatever streams they are on: such a call on another stream than the last one's
 *     waits on the device (an event recorded on that stream when the later call is issued, hipStreamWaitEvent) for that one
 *     and for what its stream has been given since, and a host entry that reads or rewrites the maps waits for them on the
 *     host.  A later call never changes what an earlier, still pending one reads; calls that stay on one stream add no event
 *     and no wait.  (A stream should outlive the work it was given; where the last such call's stream has been destroyed, the
 *     next one waits for the whole device instead.)  famseq_bn_batch_device,
 *     famseq_bn_prior_batch_device and the side entries given d_lk use no such state: no event, no wait, and calls on
 *     different streams may overlap.
 *   - Capturing these entries into a HIP graph is not supported (uploads from staging memory the context reuses, events). */
int famseq_bn_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint8_t *d_flags,
                           double *d_post, double *d_post_single, uint8_t *d_status, void *stream);

/* Device-resident form of famseq_bn_batch_sharded, for a process that holds several GPUs (the
 * reference has no multi-GPU: family.cu:1152 binds device 0): shard g is n_sites[g] sites whose
 * arrays are already resident on ctxs[g]'s device.  One host thread per ctx enqueues the shard on
 * that ctx's own compute stream and waits for it; blocking; no collective and no copy between
 * devices.  d_flags / d_post_single / d_status may be NULL, and so may their entries.  Returns 0 or
 * the first error any ctx reported.  (Several ctxs may name the same device: rehearsal on one GPU.) */
int famseq_bn_batch_device_sharded(famseq_ctx *const *ctxs, int n_ctx, const int64_t *n_sites,
                                   const double *const *d_lk, const uint8_t *const *d_flags, double *const *d_post,
                                   double *const *d_post_single, uint8_t *const *d_status);

/* Fused call path (SURVEY.md 8(f) rows N2 + N4): what the drivers print per sequenced sample, computed on
 * the device, so that only 49*n_seq bytes per site come back instead of 48*N.
 *   input   either lk  [n_sites][N][3] fp64 (as famseq_bn_batch)
 *           or     pl16 [n_sites][n_seq][3] uint16: integer PL/GL magnitudes in VCF column order, turned
 *                  into likelihoods on the device with the reference's pow(10,-|x|/10) (file.cpp:588-590,
 *                  table filled by the host libm); 0xFFFF,0xFFFF,0xFFFF = sample missing at this site
 *                  (likelihood {1,1,1}, file.cpp:794-809); members outside seq_members are {1,1,1} (:565)
 *   seq_members[n_seq]  PED index of each sequenced sample in VCF column order (mapV2P[i] >= 0)
 *   gpp, fpp [n_sites][n_seq][3]  fabs(-10*log10(p)) of the single / BN posterior, +inf -> 99999
 *                                 (file.cpp:696-745); NaN where the site failed
 *   fgt      [n_sites][n_seq]     arg-max genotype 0/1/2 (family.cpp:636-665), -1 where the site failed
 * Any of gpp / fpp / fgt / status may be NULL.  Blocking; chunks are pipelined like famseq_bn_batch.
 * Batches served by a generated kernel run ONE kernel per chunk — its call-path form unpacks the PLs into
 * the LDS rows and turns the posterior rows into GPP / FPP / FGT while storing them; the fp64 likelihoods and
 * posteriors never exist in HBM.  The compiled-in team kernel and the lanes-per-site mode (tiny batches)
 * keep the separate unpack / posterior / Phred stages; both ways give the same bits. */
int famseq_bn_call_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16,
                         const uint8_t *flags, const int32_t *seq_members, int32_t n_seq, double *gpp, double *fpp,
                         int8_t *fgt, uint8_t *status);

/* The same call with the outputs as TEXT (SURVEY.md 8(f) rows N1 + N2): what the reference's drivers append to every
 * sample column of an output line (file.cpp:696-745) — the GPP triple, the FPP triple and the called genotype,
 * "g0,g1,g2:f0,f1,f2:0/1\t", every number as C++ `ostream << double` prints it (printf's %g: six significant digits of the
 * exact binary value, round-half-even) — formatted on the device by one more streaming kernel over the called outputs
 * while they are in HBM (csrc/io_kernels.hip text_call_kernel; csrc/g6_core.h is the digit code it shares with the host
 * formatter).  The sixty %g conversions per ten-member site were the slowest stage of the command line (0.74 of its 0.88 s
 * loop per 3 M sites on 16 host threads); with this entry the host copies one record per sample.
 *   text [n_sites][n_seq][FAMSEQ_TEXT_STRIDE]  one record per (site, sequenced sample) in VCF column order: the characters
 *        from byte 0, their count (<= 76) in byte FAMSEQ_TEXT_STRIDE - 1, zeros between.  Records of a site whose
 *        status has bit 0 or 1 set hold no number to print (the drivers write ":NA:NA:NA" there, file.cpp:607-620).
 * Other arguments, chunking and kernels as famseq_bn_call_batch; 80 n_seq + 1 bytes per site come back. */
#define FAMSEQ_TEXT_STRIDE 80
int famseq_bn_call_text_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16,
                              const uint8_t *flags, const int32_t *seq_members, int32_t n_seq, char *text, uint8_t *status);

/* The call path on DEVICE buffers already resident on ctx's device: enqueues on `stream` (a hipStream_t; NULL = the default stream)
 * and returns without synchronising (the stream rule at famseq_bn_batch_device; this entry uses the context's column maps,
 * argument block and scratch); nothing crosses the host link.  Exactly one of d_lk / d_pl16; seq_members is a HOST array
 * (uploaded on `stream` when it changes); any of d_gpp / d_fpp / d_fgt / d_status / d_text may be NULL (d_text: 16-byte aligned,
 * [n_sites][n_seq][FAMSEQ_TEXT_STRIDE]).  The same kernels as famseq_bn_call_batch / famseq_bn_call_text_batch; batches they do not
 * serve fused go through scratch rows this context keeps (grown on demand). */
int famseq_bn_call_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                const uint8_t *d_flags, const int32_t *seq_members, int32_t n_seq, double *d_gpp, double *d_fpp,
                                int8_t *d_fgt, uint8_t *d_status, char *d_text, void *stream);

/* ---- trio posteriors and de novo mutations ------------------------------------------------------------
 * What the marginals cannot say: is a child's variant a de novo mutation?  That needs the JOINT posterior of the child's and
 * both parents' genotypes, which the sum-product engine's family factors hold (the clique belief of a nuclear family, restricted
 * to one child and the parents).  Served for every pedigree the engine serves: loop-free ones of any size, and pedigrees with
 * loops up to three conditioned members; any other gets FAMSEQ_E_ARG with the engine's message.
 *   children   the members that have parents, in PED order; K = their count; child k is member children[k]
 *   joint [n_sites][K][27]  the posterior over (child k, its mother, its father) in the full pedigree network — the network
 *              the 3^N enumeration sums, with the same priors (Known flag), chrX tables and male priors and likelihoods —
 *              indexed 9 gc + 3 gm + gf (the transmission tables' order); the 27 values sum to 1
 *   dnm   [n_sites][K]      the de novo posterior: the sum of joint over the entries where the mutation-free transmission table
 *              of the child is exactly 0 (autosomes: the autosomal table at mutation rate 0; chrX: the son's or the daughter's),
 *              i.e. the posterior probability that the child's genotype is Mendelian-inconsistent with its parents'.  Exactly 0.0
 *              at mutation rate 0.
 *   status [n_sites]        0 OK; 1 the single-posterior failure rule of famseq_bn_batch (a lk * prior row sum <= 0: the
 *              drivers print such a site as NA); 2 the network's total weight is <= 0.  There is no -LRC shortcut: every site
 *              runs the full network.  Wherever status != 0, joint and dnm are NaN.
 * The kernel is generated per pedigree and output form (dnm only, joint only, both: chosen from which outputs are given) and
 * compiled on the first trio call, or ahead through famseq_set_option "trio_kernels" (1 dnm, 2 joint, 3 both); nothing of it
 * exists before.  famseq_plan_json: "trio_code_object", "trio_variant", "trio_children". */

/* K, and the children's member indices in idx[K] (idx may be NULL).  FAMSEQ_E_ARG on a pedigree the engine does not serve. */
int famseq_trio_children(famseq_ctx *ctx, int32_t *idx);

/* Host buffers, blocking, chunked and pipelined like famseq_bn_call_batch.  Exactly one of lk [n_sites][N][3] / pl16
 * [n_sites][n_seq][3] (packed PLs in VCF column order, seq_members[n_seq] their PED indices, as famseq_bn_call_batch: unpacked
 * on the device by the same stage); seq_members / n_seq are ignored with lk.  Any of joint / dnm / status may be NULL. */
int famseq_trio_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                      int32_t n_seq, const uint8_t *flags, double *joint, double *dnm, uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array): enqueues on `stream` (a hipStream_t;
 * NULL = the default stream) and returns without synchronising (the stream rule at famseq_bn_batch_device).  Packed input goes through likelihood rows this context keeps. */
int famseq_trio_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                             const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, double *d_joint, double *d_dnm,
                             uint8_t *d_status, void *stream);

/* ---- the joint MAP genotype configuration ---------------------------------------------------------------
 * FGT is each member's own most probable genotype; member by member those need not form a configuration that has any
 * probability at all (at mutation rate 0 they can be Mendelian-inconsistent).  This is the other answer: the single most probable
 * genotype assignment of the whole pedigree and its posterior probability, by max-product message passing (with back-pointers)
 * on the sum-product engine's graph.  Exact, O(27 N) per site, for every pedigree that engine serves: loop-free ones of any size,
 * loops up to three conditioned members; any other gets FAMSEQ_E_ARG with the engine's message.  With w(g) = 1e7 * prod_m
 * f_m(g_m | g_mother, g_father), the weight the 3^N enumeration gives a configuration (priors by the Known flag, chrX tables and
 * male priors by the chrX flag):
 *   map_gt  [n_sites][N] int8   g* = argmax_g w(g): 0 / 1 / 2 per member, PED order
 *   map_post[n_sites]    fp64   w(g*) / sum_g w(g)
 *   status  [n_sites]           0 OK; 1 the single-posterior failure rule of famseq_bn_batch; 2 the total or the maximum weight
 *              is <= 0.  There is no -LRC shortcut.  Wherever status != 0, map_gt is -1 and map_post NaN.
 * Ties: every arg-max of the kernel scans genotypes in the order 0, 1, 2 (parent pairs in the order 3 gm + gf; conditioned
 * members' assignments in loop order) and replaces on strictly greater only, so the result is a function of the input.  Two
 * configurations whose weights differ only by rounding may compare differently under another order of multiplication (an
 * enumeration's): what is guaranteed against such a reference is the weight of the returned configuration, not its identity.
 * The kernel is compiled on the first MAP call, or ahead through famseq_set_option "map_kernels" = 1 (a plan-only context
 * generates and cross-compiles it).  famseq_plan_json: "map_code_object", "map_variant". */

/* Host buffers, blocking, chunked and pipelined; inputs as famseq_trio_batch (exactly one of lk / pl16).  Any of map_gt /
 * map_post / status may be NULL. */
int famseq_map_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                     int32_t n_seq, const uint8_t *flags, int8_t *map_gt, double *map_post, uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array): enqueues on `stream` (a hipStream_t;
 * NULL = the default stream) and returns without synchronising (the stream rule at famseq_bn_batch_device). */
int famseq_map_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                            const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, int8_t *d_map_gt,
                            double *d_map_post, uint8_t *d_status, void *stream);

/* ---- founder priors per site -----------------------------------------------------------------------------------------
 * famseq_bn_batch with the founders' genotype prior given per site — a population allele frequency, say — instead of the
 * model's genoProbN / genoProbK (genoProbXN / genoProbXK) rows.  prior[n_sites][6], required: doubles 0-2 are the prior
 * (genotypes 0 / 1 / 2) of female founders and of every founder at an autosomal site, doubles 3-5 the prior of male founders
 * at a chrX site; they are read at sites with FAMSEQ_FLAG_CHRX only.  Entries must be finite and >= 0 (the host entry checks:
 * FAMSEQ_E_ARG); a row need not sum to 1.  FAMSEQ_FLAG_KNOWN is not read; FAMSEQ_FLAG_CHRX selects the transmission tables and
 * the male row as it does for famseq_bn_batch.  Layouts and statuses are famseq_bn_batch's: status 1 where lk * prior sums
 * to <= 0 for any member (so an all-zero row fails its site), 2 where a network row sum is <= 0, 0x80 the -LRC shortcut;
 * failed rows are NaN.  Given rows that equal the model's constants the outputs are, bit for bit, those of the sum-product
 * engine's famseq_bn_batch.
 * Served by the site-prior form of the sum-product kernel whatever "engine" says, for every pedigree that engine serves
 * (FAMSEQ_E_ARG with its message otherwise).  The kernel is compiled on the first call, or ahead through famseq_set_option
 * "prior_kernels" = 1 (a plan-only context generates and cross-compiles it); it takes the variant the sum-product kernel
 * takes for the pedigree (its measured one, "pick_elim" / "tune", where there is one; else the winner of that
 * kernel's spill contest, which the first call on an unmeasured pedigree compiles too where the cache does not hold it).  famseq_plan_json: "prior_code_object", "prior_variant". */

/* Host buffers, blocking, chunked and pipelined (a chunk's prior rows travel with its likelihoods).  post_single and status
 * may be NULL. */
int famseq_bn_prior_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint8_t *flags, const double *prior,
                          double *post, double *post_single, uint8_t *status);

/* The same on device buffers resident on ctx's device: enqueues on `stream` (a hipStream_t; NULL = the default stream) and
 * returns without synchronising (the stream rule at famseq_bn_batch_device).  Nothing is checked of d_prior's contents. */
int famseq_bn_prior_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint8_t *d_flags,
                                 const double *d_prior, double *d_post, double *d_single, uint8_t *d_status, void *stream);

/* The call path under site priors (`FamSeq vcf -afTag`): famseq_bn_call_batch's inputs and called outputs (or, with `text`
 * given, famseq_bn_call_text_batch's records instead of gpp / fpp / fgt) with one prior row per site as above.  Per chunk the
 * separate stages on the device: PL unpack, the site-prior kernel, Phred scaling and genotype call, text; there is no fused
 * call-path form of the site-prior kernel. */
int famseq_bn_prior_call_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const uint8_t *flags,
                               const double *prior, const int32_t *seq_members, int32_t n_seq, double *gpp, double *fpp, int8_t *fgt,
                               char *text, uint8_t *status);

/* ---- founder priors per site for the trio posteriors and the joint MAP call -------------------------------------------
 * famseq_trio_batch and famseq_map_batch with the founders' genotype prior given per site: prior[n_sites][6], required, laid
 * out, read (the male half at chrX sites only; FAMSEQ_FLAG_KNOWN not read) and checked by the host entries (finite, >= 0, else
 * FAMSEQ_E_ARG naming the site) exactly as for famseq_bn_prior_batch.  The de novo posterior is the output that depends most
 * on that prior: the evidence that makes a de novo call at a singleton is, at a common variant, a missed parental heterozygote.
 * Outputs, layouts and statuses are the plain entries' with the prior row in the place of genoProb*: status 1 where lk * prior
 * sums to <= 0 for any member (an all-zero row fails its site), 2 where the network's total weight (MAP: or the maximum) is <= 0,
 * no shortcut; joint / dnm / map_post NaN and map_gt -1 wherever status != 0.  The de novo mask depends on the transmission
 * tables only and is unchanged.  Given rows that equal the model's constants the outputs are, bit for bit, famseq_trio_batch's
 * and famseq_map_batch's.
 * The kernels (famseq_trio_prior per output form, famseq_map_prior) are compiled on the first call, or ahead through
 * famseq_set_option "trio_prior_kernels" (1 dnm, 2 joint, 3 both) / "map_prior_kernels" = 1 (a plan-only context generates and
 * cross-compiles them); each takes the variant its plain sibling's contest takes for the pedigree.  famseq_plan_json:
 * "trio_prior_code_object", "trio_prior_variant" (the form asked for last), "map_prior_code_object", "map_prior_variant". */

/* Host buffers, blocking, chunked and pipelined (a chunk's prior rows travel with its likelihoods); the other arguments as
 * famseq_trio_batch / famseq_map_batch. */
int famseq_trio_prior_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                            int32_t n_seq, const uint8_t *flags, const double *prior, double *joint, double *dnm, uint8_t *status);
int famseq_map_prior_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                           int32_t n_seq, const uint8_t *flags, const double *prior, int8_t *map_gt, double *map_post, uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array): enqueue on `stream` (a hipStream_t;
 * NULL = the default stream) and return without synchronising (the stream rule at famseq_bn_batch_device).  Nothing is checked of d_prior's contents. */
int famseq_trio_prior_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                   const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                   double *d_joint, double *d_dnm, uint8_t *d_status, void *stream);
int famseq_map_prior_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                  const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                  int8_t *d_map_gt, double *d_map_post, uint8_t *d_status, void *stream);

/* ---- the evidence: the site's likelihood under the pedigree, and the family's variant quality ---------------------------
 * The third standard query on the pedigree network, beside the marginals (famseq_bn_batch, famseq_trio_batch) and the most
 * probable assignment (famseq_map_batch): the total weight itself, which every other kernel forms, divides by and drops.  With
 * w(g) = prod_m f_m(g_m | g_mother, g_father), f = prior * lk for a founder and T[g | gm, gf] * lk for a child (priors by the
 * Known flag, chrX tables and male priors by the chrX flag; no 1e7):
 *   loglik [n_sites] fp64   log10 sum_g w(g): the data's likelihood under the pedigree and the model.  Summed over sites it
 *              compares mutation rates, founder priors and pedigree hypotheses (a sample swap, non-paternity).  It may be
 *              positive: likelihood rows and priors need not sum to 1.
 *   pref   [n_sites] fp64   w(0, ..., 0) / sum_g w(g): the posterior probability that every member is hom-ref, i.e. that the
 *              site is not variant in this family at all.  Not a product of the members' marginals, which are not independent.
 *              0.0 where the hom-ref configuration has no weight.
 *   status [n_sites]        0 OK; 1 the single-posterior failure rule of famseq_bn_batch; 2 the total weight is <= 0 or not
 *              finite.  There is no -LRC shortcut.  Wherever status != 0, loglik and pref are NaN.
 * The sum pass of famseq_map_batch on the sum-product engine's graph, O(27 N) per site, for every pedigree that engine serves:
 * loop-free ones of any size, loops up to three conditioned members; any other gets FAMSEQ_E_ARG with the engine's message.
 * The kernel is compiled on the first call, or ahead through famseq_set_option "evidence_kernels" = 1 (a plan-only context
 * generates and cross-compiles it).  famseq_plan_json: "evidence_code_object", "evidence_variant", "evidence_block_threads" (the
 * sites a workgroup takes per loop trip: one per lane). */

/* Host buffers, blocking, chunked and pipelined; inputs as famseq_map_batch (exactly one of lk / pl16, seq_members / n_seq for
 * packed input).  Any of loglik / pref / status may be NULL. */
int famseq_evidence_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                          int32_t n_seq, const uint8_t *flags, double *loglik, double *pref, uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array): enqueues on `stream` (a hipStream_t;
 * NULL = the default stream) and returns without synchronising (the stream rule at famseq_bn_batch_device). */
int famseq_evidence_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                 const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, double *d_loglik, double *d_pref,
                                 uint8_t *d_status, void *stream);

/* With the founders' genotype prior given per site: prior[n_sites][6], required, laid out, read (the male half at chrX sites
 * only; FAMSEQ_FLAG_KNOWN not read) and checked by the host entry (finite, >= 0, else FAMSEQ_E_ARG naming the site) exactly as
 * for famseq_map_prior_batch.  Given rows that equal the model's constants the outputs are, bit for bit, famseq_evidence_batch's.
 * The kernel (famseq_evidence_prior) is compiled on the first call or ahead through "evidence_prior_kernels" = 1 and takes the
 * variant its plain sibling's contest takes.  famseq_plan_json: "evidence_prior_code_object", "evidence_prior_variant".
 * Nothing is checked of d_prior's contents. */
int famseq_evidence_prior_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                int32_t n_seq, const uint8_t *flags, const double *prior, double *loglik, double *pref,
                                uint8_t *status);
int famseq_evidence_prior_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                       const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                       double *d_loglik, double *d_pref, uint8_t *d_status, void *stream);

/* ---- leave-one-out posteriors and per-member fit: what the relatives alone say of a member ----------------------------------
 * Every other entry folds a member's own reads into that member's answer.  This one leaves them out, for every member at once,
 * from the messages of one pass over the network (with w as for the evidence):
 *   loo  [n_sites][N][3] fp64   loo[i][a] = P(g_i = a | the likelihood rows of every member but i), normalised over a: member
 *              i's marginal had its row been (1, 1, 1).  For a member whose row is all ones (not sequenced) its posterior.
 *              The own row is left out of the product, never divided out: an exact 0 in a row costs nothing.
 *   fit  [n_sites][N] fp64      sum_a loo[i][a] * lk[i][a] = Z / Z_-i, Z_-i the total weight with row i set to ones: the
 *              predictive likelihood of member i's row given its relatives, linear (no logarithm), in the units of the row as
 *              given.  Summed in logs over the sites of a file it is the per-sample statistic for sample swaps, contamination
 *              and Mendelian errors.  0.0 where the row is impossible given the relatives: a result, not a failure.  Where
 *              Z > 0, famseq_bn_batch's post[i][a] = loo[i][a] * lk[i][a] / fit[i].
 *   status [n_sites]        0 OK; 1 the single-posterior failure rule of famseq_bn_batch; 2 some member's unnormalised cavity
 *              row sums to <= 0 or is not finite.  There is no -LRC shortcut.  Wherever status != 0, loo and fit of the whole
 *              site are NaN.
 * O(27 N) per site on the sum-product engine's graph, for every pedigree that engine serves: loop-free ones of any size, loops
 * up to three conditioned members; any other gets FAMSEQ_E_ARG with the engine's message.  The kernel is compiled on the first
 * call, or ahead through famseq_set_option "loo_kernels" = 1 (a plan-only context generates and cross-compiles it).
 * famseq_plan_json: "loo_code_object", "loo_variant", "loo_block_threads" (the sites a workgroup takes per loop trip: one per
 * lane). */

/* Host buffers, blocking, chunked and pipelined; inputs as famseq_map_batch (exactly one of lk / pl16, seq_members / n_seq for
 * packed input).  Any of loo / fit / status may be NULL. */
int famseq_loo_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                     int32_t n_seq, const uint8_t *flags, double *loo, double *fit, uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array): enqueues on `stream` (a hipStream_t;
 * NULL = the default stream) and returns without synchronising (the stream rule at famseq_bn_batch_device). */
int famseq_loo_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16, const int32_t *seq_members,
                            int32_t n_seq, const uint8_t *d_flags, double *d_loo, double *d_fit, uint8_t *d_status, void *stream);

/* With the founders' genotype prior given per site: prior[n_sites][6], required, laid out, read (the male half at chrX sites
 * only; FAMSEQ_FLAG_KNOWN not read) and checked by the host entry (finite, >= 0, else FAMSEQ_E_ARG naming the site) exactly as
 * for famseq_map_prior_batch.  Given rows that equal the model's constants the outputs are, bit for bit, famseq_loo_batch's.
 * The kernel (famseq_loo_prior) is compiled on the first call or ahead through "loo_prior_kernels" = 1 and takes the variant
 * its plain sibling's contest takes.  famseq_plan_json: "loo_prior_code_object", "loo_prior_variant".  Nothing is checked of
 * d_prior's contents. */
int famseq_loo_prior_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                           int32_t n_seq, const uint8_t *flags, const double *prior, double *loo, double *fit, uint8_t *status);
int famseq_loo_prior_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                  const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior, double *d_loo,
                                  double *d_fit, uint8_t *d_status, void *stream);

/* ---- genotype-pattern posteriors ---------------------------------------------------------------------------------------
 * A pattern gives every member a set of allowed genotypes; its posterior is the probability, given everybody's data, that
 * every member's genotype lies in its set:  P(g_i in A_i for every i | data) = Z_A / Z,  Z_A being the network's total weight
 * with the disallowed entries of every likelihood row set to zero.  (Members' marginals are not independent: the product of
 * their P(g_i in A_i) is not this number.)  Segregation with a phenotype is two such patterns: "dominant", the affected carry
 * the variant (mask 6) and the unaffected do not (1); "recessive", the affected are hom-alt (4) and nobody else named is (3).
 *   masks [n_patterns][N]   one byte per member in PED order: bit g set = genotype g allowed.  7 leaves the member
 *              unconstrained; 0 is legal and makes the pattern impossible.  The same for every site of the call.
 *   n_patterns              1 .. FAMSEQ_MAX_PATTERNS.
 *   pat_post [n_sites][n_patterns]   Z_m / Z, in [0, 1]: exactly 1.0 for a pattern of 7s, exactly 0.0 for a pattern without
 *              weight (a result, not a failure).
 *   loglik [n_sites]        famseq_evidence_batch's: log10 of the site's likelihood under the pedigree.
 *   status [n_sites]        0 OK; 1 the single-posterior failure rule of famseq_bn_batch, applied to the rows as given; 2 the
 *              total weight Z is <= 0 or not finite.  Wherever status != 0, pat_post and loglik of the site are NaN.
 * One kernel launch reads a site's rows once and runs the sum pass n_patterns + 1 times on them.  Served by the sum-product
 * engine's graph as famseq_evidence_batch is, whatever the context's engine; compiled on the first call or ahead through
 * famseq_set_option "pattern_kernels" = 1.  famseq_plan_json: "pattern_code_object", "pattern_variant".
 * FAMSEQ_E_ARG, with a message: n_patterns outside 1 .. FAMSEQ_MAX_PATTERNS, masks NULL, (host entries) a mask byte > 7. */
#define FAMSEQ_MAX_PATTERNS 32

/* Host buffers, blocking, chunked and pipelined; inputs as famseq_evidence_batch.  masks is a host array, staged by the library.
 * Any of pat_post / loglik / status may be NULL. */
int famseq_pattern_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                         int32_t n_seq, const uint8_t *flags, const uint8_t *masks, int32_t n_patterns, double *pat_post,
                         double *loglik, uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array), d_masks among them — it must stay valid
 * and unchanged until the kernel has run, and only its low three bits per byte are read: enqueues on `stream` (a hipStream_t;
 * NULL = the default stream) and returns without synchronising (the stream rule at famseq_bn_batch_device). */
int famseq_pattern_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const uint8_t *d_masks,
                                int32_t n_patterns, double *d_pat_post, double *d_loglik, uint8_t *d_status, void *stream);

/* With the founders' genotype prior given per site: prior[n_sites][6], as for famseq_evidence_prior_batch.  Given rows that equal
 * the model's constants the outputs are, bit for bit, famseq_pattern_batch's.  "pattern_prior_kernels" = 1 builds the kernel
 * (famseq_pattern_prior) ahead; famseq_plan_json: "pattern_prior_code_object", "pattern_prior_variant". */
int famseq_pattern_prior_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                               int32_t n_seq, const uint8_t *flags, const double *prior, const uint8_t *masks, int32_t n_patterns,
                               double *pat_post, double *loglik, uint8_t *status);
int famseq_pattern_prior_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                      const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                      const uint8_t *d_masks, int32_t n_patterns, double *d_pat_post, double *d_loglik,
                                      uint8_t *d_status, void *stream);

/* ---- exact joint posterior draws -----------------------------------------------------------------------------------------
 * n_draws joint genotype configurations per site, each drawn from the posterior of the whole pedigree: for any statistic of the
 * family that is not one of the closed forms above (carrier counts, transmitted alleles, burden over sites), with the family's
 * dependence intact.  One collect pass of the sum-product messages, then per draw a backward pass that chooses where the MAP
 * kernel maximises: exact, independent draws, no burn-in, for every pedigree the sum-product engine serves.
 *   samp_gt  [n_sites][n_draws][N] int8   configuration g drawn with probability w(g) / Z (w as for the evidence), PED order.
 *   samp_post[n_sites][n_draws] fp64      w(g) / Z of the configuration drawn.
 *   status   [n_sites]      0 OK; 1 the single-posterior failure rule of famseq_bn_batch; 2 the total weight Z is <= 0 or not
 *              finite.  Wherever status != 0 every genotype of the site is -1 and every samp_post NaN.  No -LRC shortcut.
 *   seed, site_base, n_draws   Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (i & 0xffffffff, i >> 32, k, j):
 *              i = site_base + the site's position in the call, k the draw, j the block; word w of the stream of (site, draw)
 *              is element w % 4 of block w / 4 and becomes u = (word + 0.5) 2^-32.  A draw is a function of the pedigree, the
 *              site's inputs, seed, i and k alone: not of the batch, the chunking, the launch or n_draws (draw 3 of 4 is draw 3
 *              of 32).  A caller that splits a batch passes each part its first site's index as site_base and gets the whole
 *              batch's rows.  One decision resolves 2^-32 of probability; a term of exactly 0 is never drawn (at mutation rate
 *              0 every draw is Mendelian-consistent).  n_draws: 1 .. FAMSEQ_MAX_DRAWS; site_base >= 0.
 * The kernel (famseq_sample) is compiled on the first call or ahead through famseq_set_option "sample_kernels" = 1;
 * famseq_plan_json: "sample_code_object", "sample_variant".  FAMSEQ_E_ARG, with a message and before the device is asked for:
 * n_draws outside 1 .. FAMSEQ_MAX_DRAWS, site_base < 0.  Pedigrees beyond about a hundred members, whose messages do not fit
 * the lanes' LDS rows, get FAMSEQ_E_HIP with the generator's message. */
#define FAMSEQ_MAX_DRAWS 256

/* Host buffers, blocking, chunked and pipelined; inputs as famseq_map_batch.  Any of samp_gt / samp_post / status may be NULL. */
int famseq_sample_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                        int32_t n_seq, const uint8_t *flags, uint64_t seed, int64_t site_base, int32_t n_draws, int8_t *samp_gt,
                        double *samp_post, uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array): enqueues on `stream` (a hipStream_t;
 * NULL = the default stream) and returns without synchronising (the stream rule at famseq_bn_batch_device). */
int famseq_sample_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                               const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, uint64_t seed, int64_t site_base,
                               int32_t n_draws, int8_t *d_samp_gt, double *d_samp_post, uint8_t *d_status, void *stream);

/* With the founders' genotype prior given per site: prior[n_sites][6], as for famseq_map_prior_batch.  Given rows that equal the
 * model's constants the outputs are, bit for bit, famseq_sample_batch's.  "sample_prior_kernels" = 1 builds the kernel
 * (famseq_sample_prior) ahead; famseq_plan_json: "sample_prior_code_object", "sample_prior_variant". */
int famseq_sample_prior_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                              int32_t n_seq, const uint8_t *flags, const double *prior, uint64_t seed, int64_t site_base,
                              int32_t n_draws, int8_t *samp_gt, double *samp_post, uint8_t *status);
int famseq_sample_prior_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                     const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                     uint64_t seed, int64_t site_base, int32_t n_draws, int8_t *d_samp_gt, double *d_samp_post,
                                     uint8_t *d_status, void *stream);

/* The generator of the entries above, one block: Philox4x32-10 of counter ctr under key -> out (Random123's known answers). */
void famseq_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

/* ---- the founders' allele frequency by maximum likelihood ---------------------------------------------------------------
 * Parameter learning: the site-prior entries above take the founders' allele frequency from outside; this one estimates it
 * from the family's own reads, by EM on the pedigree network, and reports the likelihood ratio against "no founder carries
 * the allele", a variant statistic that rests on no prior at all.
 * The founders' genotypes at a site are Hardy-Weinberg draws at allele frequency q: with p = 1 - q the rows famseq_hwe_priors
 * makes, (p p, 2 q p, q q) for female founders and every founder off chrX, (p, 0, q) for male founders at a chrX site.  Z(q)
 * is the network's total weight under those rows, m_f(q) founder f's marginal row.  One step from q:
 *     A = sum over the founders, in PED order, of (m_f1 + 2 m_f2) / (m_f0 + m_f1 + m_f2)
 *         [a male founder at a chrX site: m_f2 / (m_f0 + m_f1 + m_f2)]
 *     C = 2 (founders)   [at a chrX site: 2 (female founders) + (male founders)]
 *     q' = min(A / C, 1.0)
 *   af0 [n_sites]        the start values, each in [0, 1]; required.
 *   n_iter               the steps T, 0 .. FAMSEQ_MAX_AF_ITER.  No early exit and no convergence test: the trip count is the
 *              call's, and the result is "q after T steps", a function of the site's inputs alone.
 *   af [n_sites]         q_T; T = 0 returns af0's bits.
 *   loglik [n_sites][2]  [0] log10 Z(q_T) on famseq_evidence_batch's scale — at T = 0 famseq_evidence_prior_batch's bits on
 *              famseq_hwe_priors(af0); it does not decrease with T.  [1] the same at q = 0, where every founder is hom-ref: -inf
 *              where the data exclude that, which is a result, not a failure.  [0] - [1] is the log10 likelihood ratio for
 *              "the allele is present among the founders".
 *   status [n_sites]     0 OK; 1 the single-posterior failure rule of famseq_bn_batch under af0's rows (what
 *              famseq_evidence_prior_batch says of famseq_hwe_priors(af0)); 2 an af0 outside [0, 1] (device entry; the host
 *              entry refuses the call), a Z(q_t), t = 0 .. T, that is <= 0 or not finite, or a founder's row sum that is.
 *              Wherever status != 0, af and both loglik entries are NaN.  FAMSEQ_FLAG_KNOWN is not read.
 * Chaining: T = a, then T = b from the first call's af, gives the bits of one call with T = a + b.
 * One kernel launch reads a site's rows once and runs T + 2 sum passes on them (the founders' marginals in T of them).  Served
 * by the sum-product engine's graph as famseq_evidence_batch is, whatever the context's engine; the kernel (famseq_af) is
 * compiled on the first call or ahead through famseq_set_option "af_kernels" = 1.  famseq_plan_json: "af_code_object",
 * "af_variant".  The prior is the unknown here: there is no site-prior form.
 * FAMSEQ_E_ARG, with a message and before the device is asked for: n_iter outside 0 .. FAMSEQ_MAX_AF_ITER, af0 NULL, (host
 * entry) the first af0[s] that is not a finite number in [0, 1], named by its site index. */
#define FAMSEQ_MAX_AF_ITER 64

/* Host buffers, blocking, chunked and pipelined; inputs as famseq_evidence_batch.  Any of af / loglik / status may be NULL. */
int famseq_af_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                    int32_t n_seq, const uint8_t *flags, const double *af0, int32_t n_iter, double *af, double *loglik,
                    uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array), d_af0 among them — nothing is checked
 * of its contents: enqueues on `stream` (a hipStream_t; NULL = the default stream) and returns without synchronising (the stream rule at famseq_bn_batch_device). */
int famseq_af_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16, const int32_t *seq_members,
                           int32_t n_seq, const uint8_t *d_flags, const double *d_af0, int32_t n_iter, double *d_af,
                           double *d_loglik, uint8_t *d_status, void *stream);

/* ---- relabelling evidence: which sample-to-member labelling fits the pedigree ---------------------------------------------
 * Every query above takes the labelling of the samples for granted.  An assignment a[N] says, for every member p in PED order,
 * which member's likelihood row it is given: a[p] in 0 .. N-1, or -1 for "no data", the row (1, 1, 1).  It need not be a
 * permutation (a row may be used twice); the identity is a[p] = p.  Z_a is the network's total weight, as famseq_evidence_batch
 * forms it, with member p's row replaced by row a[p] of the site as given.  The substitution happens before anything else sees
 * the row: the founders' priors, the site's own prior rows, the male chrX row and a conditioned member's factor follow
 * unchanged, and a female's row handed to a male at a chrX site loses its heterozygote entry as a male's own row would.
 * Summed over sites, alt_loglik[.][j] - loglik is the log10 Bayes factor of relabelling j against the labelling as given.
 *   assign [n_assign][N]    int32, the same for every site of the call.
 *   n_assign                1 .. FAMSEQ_MAX_RELABEL (the transpositions of eleven samples are 55).
 *   alt_loglik [n_sites][n_assign]   log10 Z_a on famseq_evidence_batch's scale: bit for bit that entry's loglik on the rows
 *              rearranged on the host wherever that call has status 0, and loglik's bits for an identity row.  Not clamped:
 *              -inf where Z_a is exactly 0 (at mutation rate 0 a Mendel-impossible relabelling; a male at a chrX site handed
 *              (0, x, 0)), which is a result, not a failure; for rows in [0, 1] finite or -inf.  A column's value depends
 *              neither on n_assign nor on the other rows of assign.
 *   loglik [n_sites]        the identity's value: famseq_evidence_batch's bits.
 *   status [n_sites]        0 OK; 1 the single-posterior failure rule of famseq_bn_batch, applied to the rows as given; 2 the
 *              as-given total weight Z is <= 0 or not finite.  Wherever status != 0, alt_loglik and loglik of the site are NaN.
 *              There is no -LRC shortcut.
 * One kernel launch reads a site's rows once and runs the sum pass n_assign + 1 times on them.  Served by the sum-product
 * engine's graph as famseq_evidence_batch is, whatever the context's engine; compiled on the first call or ahead through
 * famseq_set_option "relabel_kernels" = 1.  famseq_plan_json: "relabel_code_object", "relabel_variant".
 * FAMSEQ_E_ARG, with a message and before the device is asked for: n_assign outside 1 .. FAMSEQ_MAX_RELABEL, assign NULL, (host
 * entries) the first entry outside -1 .. N-1, named by assignment and member. */
#define FAMSEQ_MAX_RELABEL 64

/* Host buffers, blocking, chunked and pipelined; inputs as famseq_evidence_batch.  assign is a host array, staged by the library.
 * Any of alt_loglik / loglik / status may be NULL; without alt_loglik only the identity pass runs. */
int famseq_relabel_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                         int32_t n_seq, const uint8_t *flags, const int32_t *assign /*[n_assign][N]*/, int32_t n_assign,
                         double *alt_loglik, double *loglik, uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array), d_assign among them — it must stay valid
 * and unchanged until the kernel has run, and nothing is checked of its contents: the kernel takes every entry outside
 * 0 .. N-1 as -1 ("no data"), so it never reads outside the site's row.  Enqueues on `stream` (a hipStream_t; NULL = the
 * default stream) and returns without synchronising (the stream rule at famseq_bn_batch_device). */
int famseq_relabel_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const int32_t *d_assign,
                                int32_t n_assign, double *d_alt_loglik, double *d_loglik, uint8_t *d_status, void *stream);

/* With the founders' genotype prior given per site: prior[n_sites][6], as for famseq_evidence_prior_batch.  Given rows that equal
 * the model's constants the outputs are, bit for bit, famseq_relabel_batch's.  "relabel_prior_kernels" = 1 builds the kernel
 * (famseq_relabel_prior) ahead; famseq_plan_json: "relabel_prior_code_object", "relabel_prior_variant". */
int famseq_relabel_prior_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                               int32_t n_seq, const uint8_t *flags, const double *prior, const int32_t *assign, int32_t n_assign,
                               double *alt_loglik, double *loglik, uint8_t *status);
int famseq_relabel_prior_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                      const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                      const int32_t *d_assign, int32_t n_assign, double *d_alt_loglik, double *d_loglik,
                                      uint8_t *d_status, void *stream);

/* ---- the mutation-rate likelihood profile: which rate the data support --------------------------------------------------------
 * The network has two kinds of parameters.  The founders' prior is given per site (the *_prior_batch entries) or learned
 * (famseq_af_batch); the mutation rate behind the transmission tables is fixed when the context is made.  These entries give, for
 * up to FAMSEQ_MAX_RATES rates at once, the site's likelihood under each.  A rate's factor table is the context's own
 * (4 flag combinations x 4 member kinds x 27 doubles, FAMSEQ_RATE_TABLE_DOUBLES in all) with the three transmission tables
 * replaced by famseq_transmission_tables(rate); Z_r is the network's total weight, as famseq_evidence_batch forms it, with the
 * children's transmission entries taken from table r.  The founders' priors stay those of the context (by the Known flag) or, in
 * the prior form, of the site's row; the single-posterior rule never reads a transmission table, so it does not depend on r.
 * With rate 0 in the grid, rate_loglik[.][r] - rate_loglik[.][r0] is the log10 Bayes factor "this site needs a mutation to be
 * explained"; summed over sites the columns give the maximum-likelihood rate.
 *   rates [n_rates]         finite numbers in [0, 1], the same for every site of the call.
 *   n_rates                 1 .. FAMSEQ_MAX_RATES.
 *   rate_loglik [n_sites][n_rates]   log10 Z_r on famseq_evidence_batch's scale.  The contract: wherever a context created from
 *              the same pedigree and priors with mrate = rates[r] answers status 0 on the same rows, rate_loglik[s][r] is that
 *              call's loglik, bit for bit.  Not clamped: -inf where Z_r is exactly 0 (rate 0 on a Mendel-impossible row with
 *              exact zeros), which is a result, not a failure.  A column's bits depend neither on n_rates nor on the other
 *              rates; two equal rates give equal bits; a rate equal to the mrate the model was made with gives loglik's bits.
 *   loglik [n_sites]        famseq_evidence_batch's bits under the context's own tables.
 *   status [n_sites]        0 OK; 1 the single-posterior failure rule of famseq_bn_batch, applied to the rows as given; 2 the
 *              context's own total weight Z is <= 0 or not finite.  Wherever status != 0, rate_loglik and loglik of the site are
 *              NaN.  There is no -LRC shortcut.
 * One kernel launch reads a site's rows once and runs the sum pass n_rates + 1 times on them, a pass's transmission entries
 * arriving through a wave-uniform pointer.  Served by the sum-product engine's graph as famseq_evidence_batch is, whatever the
 * context's engine; compiled on the first call or ahead through famseq_set_option "mutrate_kernels" = 1 (a context without a
 * device generates and cross-compiles it).  famseq_plan_json: "mutrate_code_object", "mutrate_variant".
 * FAMSEQ_E_ARG, with a message and before the device is asked for: n_rates outside 1 .. FAMSEQ_MAX_RATES, rates / d_tables NULL,
 * (host entries and famseq_rate_tables) the first rates[r] that is not a finite number in [0, 1], named by its index. */
#define FAMSEQ_MAX_RATES 32
#define FAMSEQ_RATE_TABLE_DOUBLES 432

/* tables[n_rates][FAMSEQ_RATE_TABLE_DOUBLES]: block r is the context's own factor table with the three transmission tables
 * replaced by famseq_transmission_tables(rates[r]) — what the device entries below take, once uploaded.  Block r equals, bit for
 * bit, the table of a context made with mrate = rates[r].  Works on a context without a device. */
int famseq_rate_tables(famseq_ctx *ctx, const double *rates, int32_t n_rates, double *tables);

/* Host buffers, blocking, chunked and pipelined; inputs as famseq_evidence_batch.  rates is a host array; the library builds the
 * tables (famseq_rate_tables) and stages them.  Any of rate_loglik / loglik / status may be NULL; without rate_loglik only the
 * pass on the context's own tables runs. */
int famseq_mutrate_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                         int32_t n_seq, const uint8_t *flags, const double *rates, int32_t n_rates, double *rate_loglik /*[n_sites][n_rates]*/,
                         double *loglik /*[n_sites]*/, uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array), d_tables [n_rates][432] among them — it must
 * stay valid and unchanged until the kernel has run, and nothing is checked of its contents: the kernel reads only the
 * transmission entries of a block and indexes nothing by them.  Enqueues on `stream` (a hipStream_t; NULL = the default stream)
 * and returns without synchronising (the stream rule at famseq_bn_batch_device: with d_lk no context state, no event and no wait;
 * with d_pl16 through the kept scratch rows, like every side entry). */
int famseq_mutrate_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_tables,
                                int32_t n_rates, double *d_rate_loglik, double *d_loglik, uint8_t *d_status, void *stream);

/* With the founders' genotype prior given per site: prior[n_sites][6], as for famseq_evidence_prior_batch.  Given rows that equal
 * the model's constants the outputs are, bit for bit, famseq_mutrate_batch's.  "mutrate_prior_kernels" = 1 builds the kernel
 * (famseq_mutrate_prior) ahead; famseq_plan_json: "mutrate_prior_code_object", "mutrate_prior_variant". */
int famseq_mutrate_prior_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                               int32_t n_seq, const uint8_t *flags, const double *prior, const double *rates, int32_t n_rates,
                               double *rate_loglik, double *loglik, uint8_t *status);
int famseq_mutrate_prior_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                      const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                      const double *d_tables, int32_t n_rates, double *d_rate_loglik, double *d_loglik,
                                      uint8_t *d_status, void *stream);

/* ---- phase by transmission: which parent a child's alleles came from --------------------------------------------------------
 * The marginals, the trio joint, the MAP call and the draws give a child's genotype; these entries give its phase.  For child k
 * (famseq_trio_children's order) with mother m and father f the network is famseq_evidence_batch's with the child's
 * transmission factor T(g_c | g_m, g_f) replaced by its allele-level form tm(a | g_m) * tf(b | g_f): a, b in {0 ref, 1 alt}
 * are the alleles received from mother and father, and the child's genotype is gamma(a, b).  With t(1 | g) = (mu, 1/2, 1 - mu)
 * and t(0 | g) = (1 - mu, 1/2, mu) for g = 0, 1, 2:
 *   autosome, and a daughter at a chrX site   gamma = a + b, tm = t; tf = t, at a chrX site with the g_f = 1 column 0
 *   a son at a chrX site                      gamma = 2 a, tm = t; tf(0 | g_f) = (1, 0, 1), tf(1 | .) = 0: his father gives no X
 * Summed over (a, b) with gamma(a, b) = g_c the product is the model's table (to 2.2e-16 relative; the son's exactly).
 *   origin [n_sites][K][4]  index 2 a + b: P(a, b | everybody's data); a row sums to 1.  For a son at a chrX site entries 1 and 3
 *              are 0.0.
 *   hettx  [n_sites][K][4]  (P(g_m = 1, a = 1), P(g_m = 1, a = 0), P(g_f = 1, b = 1), P(g_f = 1, b = 0)): the posterior-expected
 *              transmissions from heterozygous parents, what a transmission test sums over families.  hettx[0] + hettx[1] is
 *              P(g_m = 1 | data).  At a chrX site the father's pair is 0.0.
 *   status [n_sites]        0 OK; 1 the single-posterior failure rule of famseq_bn_batch; 2 a child's normaliser (the sum of its
 *              four unnormalised origin terms, left to right) is <= 0 or not finite.  Wherever status != 0 both outputs of the
 *              whole site are NaN.  There is no -LRC shortcut.
 * A term that holds a factor of exactly 0 is exactly 0.0: at mutation rate 0 every Mendel-impossible entry is 0.0, a result.
 * famseq_model carries tables, not a rate: mu is taken to be pcp2Xm[18], and pcp2, pcp2Xf and pcp2Xm must be, bit for bit,
 * famseq_transmission_tables(mu); otherwise FAMSEQ_E_ARG (there is no allele-level model for custom tables), said before the
 * device is asked for.  famseq_plan_json: "origin_mrate" (null for such a model).
 * Served by the sum-product engine's graph as famseq_evidence_batch is, whatever the context's engine; compiled on the first
 * call or ahead through famseq_set_option "origin_kernels" = 1 (a context without a device generates and cross-compiles it).
 * The kernel's text holds no rate: it reads the allele rows from a table the context uploads once, on the first call.
 * famseq_plan_json: "origin_code_object", "origin_variant". */
#define FAMSEQ_ALLELE_TABLE_DOUBLES 48

/* tables[2 chrX][2 child sex: 0 son, 1 daughter][2 parent: 0 mother, 1 father][2 allele][3 parent's genotype]: tm and tf above for
 * the model's mutation rate.  Works on a context without a device. */
int famseq_allele_tables(famseq_ctx *ctx, double *tables /*[FAMSEQ_ALLELE_TABLE_DOUBLES]*/);

/* Host buffers, blocking, chunked and pipelined; inputs as famseq_evidence_batch.  Any of origin / hettx / status may be NULL. */
int famseq_origin_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                        int32_t n_seq, const uint8_t *flags, double *origin /*[n_sites][K][4]*/, double *hettx /*[n_sites][K][4]*/,
                        uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array).  Enqueues on `stream` (a hipStream_t; NULL =
 * the default stream) and returns without synchronising (the stream rule at famseq_bn_batch_device: with d_lk no context state
 * beyond the allele rows, which the first call of a context uploads with a blocking copy before it enqueues anything; with
 * d_pl16 through the kept scratch rows, like every side entry). */
int famseq_origin_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                               const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, double *d_origin, double *d_hettx,
                               uint8_t *d_status, void *stream);

/* With the founders' genotype prior given per site: prior[n_sites][6], as for famseq_evidence_prior_batch.  Given rows that equal
 * the model's constants the outputs are, bit for bit, famseq_origin_batch's.  "origin_prior_kernels" = 1 builds the kernel
 * (famseq_origin_prior) ahead; famseq_plan_json: "origin_prior_code_object", "origin_prior_variant". */
int famseq_origin_prior_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                              int32_t n_seq, const uint8_t *flags, const double *prior, double *origin, double *hettx, uint8_t *status);
int famseq_origin_prior_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                     const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                     double *d_origin, double *d_hettx, uint8_t *d_status, void *stream);

/* ---- per-member genotype weights: the expectation of a product of per-member factors under the joint posterior ---------------
 * E[ prod_p w_p(g_p) | data ] = Z(lk o w) / Z(lk), for up to FAMSEQ_MAX_WEIGHTS weight tables w at once: the soft form of the
 * pattern entries' 0/1 masks.  With w_p = the penetrance (f0, f1, f2) of an affected member and 1 - f of an unaffected one it is
 * P(phenotypes | reads, pedigree) with phenocopies and incomplete penetrance; with w = t^count a moment generating function of a
 * genotype count; a phenotype likelihood folded into the evidence.
 *   weights [n_weights][N][3]   member p's weight of genotype g in table m at weights[(m * N + p) * 3 + g], the same for every
 *              site of the call; every member has a row, sequenced or not.  Finite numbers >= 0; above 1 is legal.
 *   n_weights               1 .. FAMSEQ_MAX_WEIGHTS.
 *   wt_loglik [n_sites][n_weights]   log10 Z_m on famseq_evidence_batch's scale, Z_m the network's total weight with every
 *              likelihood entry multiplied once, in double, by its weight.  The contract: wherever famseq_evidence_batch (the
 *              prior form: famseq_evidence_prior_batch) answers status 0 on the rows lk[s][p][g] * weights[m][p][g] formed in
 *              double on the host, wt_loglik[s][m] is that call's loglik, bit for bit; where it does not although this call has
 *              status 0, Z_m is exactly 0 and the entry is -inf, which is a result, not a failure.  Hence a column depends on
 *              neither n_weights nor the other tables; a table of ones gives loglik's bits; equal tables give equal bits; a 0/1
 *              table gives the Z_m of the pattern with those masks (10^(wt_loglik - loglik) is famseq_pattern_batch's posterior
 *              up to its own rounding); packed and fp64 input give the same bits.  Nothing is clamped: a Z_m that overflows
 *              gives +inf, a result.
 *   loglik [n_sites]        famseq_evidence_batch's bits on the rows as they are.
 *   status [n_sites]        0 OK; 1 the single-posterior failure rule of famseq_bn_batch, applied to the rows as given; 2 the
 *              unweighted total weight Z is <= 0 or not finite.  Wherever status != 0, wt_loglik and loglik of the site are NaN.
 *              There is no -LRC shortcut.
 * One kernel launch reads a site's rows once and runs the sum pass n_weights + 1 times on them, a pass's weights arriving
 * through a wave-uniform pointer.  Served by the sum-product engine's graph as famseq_evidence_batch is, whatever the context's
 * engine; compiled on the first call or ahead through famseq_set_option "weight_kernels" = 1 (a context without a device
 * generates and cross-compiles it).  famseq_plan_json: "weight_code_object", "weight_variant".
 * FAMSEQ_E_ARG, with a message and before the device is asked for: n_weights outside 1 .. FAMSEQ_MAX_WEIGHTS, weights /
 * d_weights NULL, (host entries) the first weight that is not a finite number >= 0 ("... weight table 2, member 1, genotype 0
 * is -0.5"), a pedigree the engine does not serve (the engine's message). */
#define FAMSEQ_MAX_WEIGHTS 32

/* Host buffers, blocking, chunked and pipelined; inputs as famseq_evidence_batch.  weights is a host array; the library checks
 * it and stages it on the stream the chunks' kernels run on.  Any of wt_loglik / loglik / status may be NULL; without wt_loglik
 * only the unweighted pass runs. */
int famseq_weight_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                        int32_t n_seq, const uint8_t *flags, const double *weights, int32_t n_weights,
                        double *wt_loglik /*[n_sites][n_weights]*/, double *loglik /*[n_sites]*/, uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array), d_weights [n_weights][N][3] among them — it
 * must stay valid and unchanged until the kernel has run, and nothing is checked of its contents: the kernel indexes nothing by
 * them.  Enqueues on `stream` (a hipStream_t; NULL = the default stream) and returns without synchronising (the stream rule at
 * famseq_bn_batch_device: with d_lk no context state, no event and no wait; with d_pl16 through the kept scratch rows, like every
 * side entry). */
int famseq_weight_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                               const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_weights,
                               int32_t n_weights, double *d_wt_loglik, double *d_loglik, uint8_t *d_status, void *stream);

/* With the founders' genotype prior given per site: prior[n_sites][6], as for famseq_evidence_prior_batch.  Given rows that equal
 * the model's constants the outputs are, bit for bit, famseq_weight_batch's.  "weight_prior_kernels" = 1 builds the kernel
 * (famseq_weight_prior) ahead; famseq_plan_json: "weight_prior_code_object", "weight_prior_variant". */
int famseq_weight_prior_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                              int32_t n_seq, const uint8_t *flags, const double *prior, const double *weights, int32_t n_weights,
                              double *wt_loglik, double *loglik, uint8_t *status);
int famseq_weight_prior_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                     const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                     const double *d_weights, int32_t n_weights, double *d_wt_loglik, double *d_loglik,
                                     uint8_t *d_status, void *stream);

/* ---- complex per-member weights: the exact distribution of an additive statistic of the family -------------------------------
 * cf[s][m] = E[ prod_p w_p(g_p) | data ] = Z(lk o w_m) / Z(lk), a complex number, for up to FAMSEQ_MAX_CWEIGHTS tables of complex
 * weights at once.  With w_p(g) = exp(i theta c_p(g)) it is the posterior characteristic function of the count sum_p c_p(g_p) at
 * theta; at the M = D + 1 roots of unity (D the count's largest value) an inverse DFT of length M gives the count's distribution,
 * well conditioned where recovering it from famseq_weight_batch's real points t^count is not.  The table conjugate to another
 * gives the conjugate result, so a caller runs the frequencies 0 .. M / 2 alone.
 *   cweights [n_tables][N][3][2]   member p's weight of genotype g in table m is the complex number at
 *              cweights[((m * N + p) * 3 + g) * 2 + {0 re, 1 im}], the same for every site of the call; every member has a row,
 *              sequenced or not.  Finite numbers.
 *   n_tables                1 .. FAMSEQ_MAX_CWEIGHTS.
 *   cf [n_sites][n_tables][2]   (Re Z_m / Z0, Im Z_m / Z0): Z0 the network's total weight on the rows as they are, Z_m with
 *              member p's likelihood entry g taken as the pair (l * w_re, l * w_im).  True divisions; nothing is clamped; a Z_m
 *              of exactly 0 gives (0.0, 0.0), which is a result.
 *   loglik [n_sites]        famseq_evidence_batch's bits on the rows as they are (the prior form: famseq_evidence_prior_batch's).
 *   status [n_sites]        0 OK; 1 the single-posterior failure rule of famseq_bn_batch, applied to the rows as given; 2 Z0 is
 *              <= 0 or not finite.  Wherever status != 0, both parts of every cf entry and loglik of the site are NaN.  There is
 *              no -LRC shortcut.
 * The contract.  Bit for bit: a column depends on neither n_tables nor the other tables; equal tables give equal bits; the table
 * conjugate to another gives the conjugate result, as numbers (every operation of the pass is odd or even in the imaginary parts;
 * an imaginary part of zero may be +0.0 in both: the sums over a looped pedigree's conditioned members start from +0.0); a table
 * whose imaginary parts are all +0.0 and whose real parts are >= 0 gives imaginary parts of exactly +0.0; if its real parts are
 * 0.0 or 1.0, cf.re is famseq_pattern_batch's pat_post of the masks with those bits, hence a table of (1, 0) entries gives
 * exactly (1.0, +0.0); packed and fp64 input give the same bits; a site's result does not depend on the batch, its chunking or
 * the launch; every variant of the kernel gives the same bits.
 * To rounding, ABSOLUTE: |cf - exact| <= 1e-12 * A, A = Z(lk o |w|) / Z(lk), which is 1 for weights of unit modulus.  Every
 * configuration's term is a product of at most about 6 N rounded factors and the terms' moduli add up to A * Z, which bounds
 * the error by 6 N * 1.1e-16 * A (3e-14 at 48 members); the terms cancel, so no relative accuracy is promised: a count
 * distribution recovered from cf is good to 1e-12 in each probability, not in each probability's digits.  For the relative
 * accuracy of a tail event (nobody carries the variant; every affected member does) famseq_pattern_batch remains the entry.
 * One kernel launch reads a site's rows once, runs the real sum pass on them and then the complex sum pass n_tables times (every
 * message a pair of doubles; transmission entries, priors and scales real), a pass's weights arriving through a wave-uniform
 * pointer.  Served by the sum-product engine's graph as famseq_evidence_batch is, whatever the context's engine: loop-free
 * pedigrees of any size, loops up to three conditioned members.  Compiled on the first call or ahead through famseq_set_option
 * "charfn_kernels" = 1 (a context without a device generates and cross-compiles it).  famseq_plan_json: "charfn_code_object",
 * "charfn_variant".
 * FAMSEQ_E_ARG, with a message and before the device is asked for: n_tables outside 1 .. FAMSEQ_MAX_CWEIGHTS, cweights /
 * d_cweights NULL, (host entries) the first entry that is not finite ("... weight table 2, member 1, genotype 0, imaginary part
 * is nan"), a pedigree the engine does not serve (the engine's message). */
#define FAMSEQ_MAX_CWEIGHTS 64

/* Host buffers, blocking, chunked and pipelined; inputs as famseq_evidence_batch.  cweights is a host array; the library checks
 * it and stages it on the stream the chunks' kernels run on.  Any of cf / loglik / status may be NULL; without cf only the real
 * pass runs. */
int famseq_charfn_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                        int32_t n_seq, const uint8_t *flags, const double *cweights /*[n_tables][N][3][2]*/, int32_t n_tables,
                        double *cf /*[n_sites][n_tables][2]*/, double *loglik /*[n_sites]*/, uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array), d_cweights among them — it must stay valid
 * and unchanged until the kernel has run, and nothing is checked of its contents: the kernel indexes nothing by them.  Enqueues
 * on `stream` (a hipStream_t; NULL = the default stream) and returns without synchronising (the stream rule at
 * famseq_bn_batch_device: with d_lk no context state, no event and no wait; with d_pl16 through the kept scratch rows, like every
 * side entry). */
int famseq_charfn_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                               const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_cweights,
                               int32_t n_tables, double *d_cf, double *d_loglik, uint8_t *d_status, void *stream);

/* With the founders' genotype prior given per site: prior[n_sites][6], as for famseq_evidence_prior_batch.  Given rows that equal
 * the model's constants the outputs are, bit for bit, famseq_charfn_batch's.  "charfn_prior_kernels" = 1 builds the kernel
 * (famseq_charfn_prior) ahead; famseq_plan_json: "charfn_prior_code_object", "charfn_prior_variant". */
int famseq_charfn_prior_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                              int32_t n_seq, const uint8_t *flags, const double *prior, const double *cweights, int32_t n_tables,
                              double *cf, double *loglik, uint8_t *status);
int famseq_charfn_prior_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                     const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                     const double *d_cweights, int32_t n_tables, double *d_cf, double *d_loglik,
                                     uint8_t *d_status, void *stream);

/* ---- max-marginals and the runner-up: the quality of the joint MAP call -----------------------------------------------------
 * famseq_map_batch gives the most probable configuration g* and its posterior; this entry says what holds the rest.  With w as
 * for famseq_map_batch and Z = sum_g w(g), by max-product message passing in both directions (no back-pointers) on the
 * sum-product engine's graph, O(27 N) per site:
 *   maxmarg [n_sites][N][3] fp64   maxmarg[p][a] = max_{g: g_p = a} w(g) / Z: the posterior of the best configuration in which
 *              member p has genotype a.  Exactly 0.0 where no configuration of positive weight has g_p = a: a result, not a
 *              failure.  The ratio of a row's two largest entries is the Phred-scalable quality of member p's joint call.
 *   top     [n_sites][2] fp64      top[0] = w(g*) / Z; top[1] = the second-largest configuration weight / Z, the runner-up's
 *              posterior (under exact ties it equals top[0]; 0.0 where one configuration holds all the weight).
 *   status  [n_sites]              0 OK; 1 the single-posterior failure rule of famseq_bn_batch; 2 the total or the maximum
 *              weight is <= 0 or not finite.  There is no -LRC shortcut.  Wherever status != 0, maxmarg and top are NaN.
 * The contract.  Bit for bit: top[0] is famseq_map_batch's map_post (the prior form: famseq_map_prior_batch's) — the kernel forms
 * the maximum and the total with that kernel's expressions; packed and fp64 input give the same bits; a site's result does not
 * depend on the batch, its chunking or the launch; every variant of the kernel gives the same bits.  To rounding (1e-9
 * relative): max_a maxmarg[p][a] = top[0] for every p (a row's maximum is formed in another order of multiplication);
 * maxmarg[p][a] <= the sum-product engine's famseq_bn_batch post[p][a], a maximum being at most the sum; maxmarg[p][a] * Z is the
 * maximum weight famseq_map_batch finds on the rows with member p's row zeroed except entry a.
 * The runner-up is the largest entry beside the rows' arg-maxes (each row scanned 0, 1, 2, replaced on strictly greater): every
 * configuration but the best differs from it at some member.
 * Served for every pedigree the engine serves: loop-free ones of any size, loops up to three conditioned members; any other gets
 * FAMSEQ_E_ARG with the engine's message.  The kernel is compiled on the first call, or ahead through famseq_set_option
 * "maxmarg_kernels" = 1 (a plan-only context generates and cross-compiles it).  famseq_plan_json: "maxmarg_code_object",
 * "maxmarg_variant". */

/* Host buffers, blocking, chunked and pipelined; inputs as famseq_map_batch (exactly one of lk / pl16).  Any of maxmarg / top /
 * status may be NULL. */
int famseq_maxmarg_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                         int32_t n_seq, const uint8_t *flags, double *maxmarg, double *top, uint8_t *status);

/* The same on device buffers resident on ctx's device (seq_members is a host array): enqueues on `stream` (a hipStream_t;
 * NULL = the default stream) and returns without synchronising (the stream rule at famseq_bn_batch_device: with d_lk no context
 * state, no event and no wait; with d_pl16 through the kept scratch rows, like every side entry). */
int famseq_maxmarg_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, double *d_maxmarg, double *d_top,
                                uint8_t *d_status, void *stream);

/* With the founders' genotype prior given per site: prior[n_sites][6], as for famseq_map_prior_batch.  Given rows that equal the
 * model's constants the outputs are, bit for bit, famseq_maxmarg_batch's.  "maxmarg_prior_kernels" = 1 builds the kernel
 * (famseq_maxmarg_prior) ahead; it takes the variant its plain sibling's contest takes.  famseq_plan_json:
 * "maxmarg_prior_code_object", "maxmarg_prior_variant".  Nothing is checked of d_prior's contents. */
int famseq_maxmarg_prior_batch(famseq_ctx *ctx, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                               int32_t n_seq, const uint8_t *flags, const double *prior, double *maxmarg, double *top, uint8_t *status);
int famseq_maxmarg_prior_batch_device(famseq_ctx *ctx, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                      const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                      double *d_maxmarg, double *d_top, uint8_t *d_status, void *stream);

/* Hardy-Weinberg rows for the site-prior entries above, on the host: prior[i] =((1-q)^2, 2q(1-q), q^2, 1-q, 0, q) for q = af[i]
 * (the male chrX row has the shape of genoProbXN: no heterozygotes). */
void famseq_hwe_priors(int64_t n, const double *af, double *prior /*[n][6]*/);

/* Diagnostic / test aid: the device formatter alone.  values[n] (host) -> out[n][16] (host): the characters of each
 * value as the text kernel prints a GPP / FPP number from byte 0, their count in byte 15; "nan" for anything outside
 * the formatter's domain, 0 and [1e-16, 999999.5). */
int famseq_format_probe(famseq_ctx *ctx, int64_t n, const double *values, char *out);

/* Diagnostic for measurement (bench.py): runs the posterior kernels' traffic shape — read one fp64 array of
 * n_doubles, write two — as a bare elementwise kernel on `stream` and returns without synchronising.  What a
 * device's memory system sustains for that shape differs between MI355X devices by 10-20 %; timing this next to
 * the kernels says how much of what is attainable THERE they reach.  Arrays must be 16-byte aligned. */
int famseq_stream_probe(famseq_ctx *ctx, int64_t n_doubles, const double *d_in, double *d_out1, double *d_out2, void *stream);

/* Page-locked host memory for the buffers handed to famseq_bn_batch / famseq_bn_call_batch: with pinned
 * buffers both directions of the host link run at their full rate at once (the callers of the reference's
 * operator own their buffers, file.cpp:565; this is how to own fast ones without linking HIP).  Returns NULL
 * when there is no device or no memory; famseq_free_pinned(NULL) is a no-op. */
void *famseq_alloc_pinned(size_t bytes);
void famseq_free_pinned(void *p);

/* get_postRlt (family.cpp:636-665) for one N x 3 posterior row block: arg-max with strict '<' starting from -1, so ties
 * resolve to the lowest genotype — here with posteriors within 1e-12 (relative) of the largest counting as ties: the
 * reference's exact ties (a 0.5 / 0.5 child at mutation rate 0) are ties to rounding only in another order of summation,
 * and the call should be the reference's there too.  The device kernels (fgt above, the text records) use the same rule. */
void famseq_call_genotypes(const double *post, int64_t n_rows, int8_t *geno);

#ifdef __cplusplus
}
#endif
#endif /* FAMSEQ_HIP_H_ */
