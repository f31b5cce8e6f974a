// capi.cpp — the C ABI of libfamseq_hip.so (see include/famseq_hip.h): the extern "C" surface and its argument checks.
//
// Replaces the host driver the reference wraps around its kernel
// (/root/reference/src/family.cu:1106-1705: per SITE 6 cudaMalloc, 5 H2D copies, one
// launch, a 4096x3N D2H copy, a host reduction and 6 cudaFree).  Here the context owns
// device memory, streams and pinned staging for its lifetime, a call moves a whole batch,
// and nothing is reduced on the host.  There is no CPU compute path in this library.
// The generated kernels are kernels.cpp's, the chunked host pipeline pipeline.cpp's; ctx.h holds what the three share.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <thread>

#include "bn_kernel.h"
#include "ctx.h"
#include "elim_codegen.h"
#include "io_kernels.h"

using namespace famseq;

namespace {

void set_err(char *err, size_t n, const std::string &msg) {
  if (err && n) {
    std::snprintf(err, n, "%s", msg.c_str());
  }
}

const char kNoDevice[] = "context was created without a device; there is no CPU path";

void validate_model(const Model &m) {
  const int n = m.n_members;
  if (n < 1) throw std::runtime_error("n_members must be >= 1 (and the member arrays given)");
  if ((int)m.mother.size() != n || (int)m.father.size() != n || (int)m.gender.size() != n || (int)m.sequenced.size() != n)
    throw std::runtime_error("member arrays do not match n_members");
  for (int i = 0; i < n; ++i) {
    const int mo = m.mother[i], fa = m.father[i];
    if ((mo < 0) != (fa < 0)) throw std::runtime_error("member with exactly one known parent");
    if (mo >= n || fa >= n) throw std::runtime_error("parent index out of range");
  }
  // nobody may be their own ancestor: generation numbers must settle within n rounds
  std::vector<int> depth(n, 0);
  for (int pass = 0; pass <= n; ++pass) {
    bool moved = false;
    for (int i = 0; i < n; ++i)
      if (m.mother[i] >= 0) {
        const int d = 1 + std::max(depth[m.mother[i]], depth[m.father[i]]);
        if (d > depth[i]) {
          depth[i] = d;
          moved = true;
        }
      }
    if (!moved) return;
  }
  throw std::runtime_error("pedigree has a member who is their own ancestor");
}

// (Re)build the plan and, on a device ctx, upload its image and the factor tables.
int refresh_plan(famseq_ctx *c) {
  if (!c->plan_dirty) return 0;
  if (!c->big) {
    try {
      c->plan = build_plan(c->model, c->opt);
    } catch (const std::exception &e) {
      return fail(c, FAMSEQ_E_ARG, std::string("plan: ") + e.what());
    }
    c->kp = make_kparams(c->plan, c->model.lc);
  }
  if (c->device >= 0) {
    HIP_TRY(c, hipSetDevice(c->device));
    double tc[4 * 4 * 27];
    build_factor_tables(c->model, tc);
    if (!c->d_tc) HIP_TRY(c, c->d_tc.alloc(sizeof tc));
    HIP_TRY(c, hipMemcpy(c->d_tc.p, tc, sizeof tc, hipMemcpyHostToDevice));
  }
  if (c->device >= 0 && !c->big) {
    std::vector<uint32_t> img = c->plan.device_image();
    for (int i = 0; i < c->model.n_members; ++i)
      img[c->kp.off_minfo + i] |= uint32_t(c->model.sequenced[i] ? 1 : 0) << 2;
    HIP_TRY(c, c->d_img.alloc(img.size() * sizeof(uint32_t)));
    HIP_TRY(c, hipMemcpy(c->d_img.p, img.data(), img.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    hipError_t e = hipSuccess;
    c->blocks_per_cu = bn_enum_blocks_per_cu(c->plan, &e);
    if (c->blocks_per_cu < 1)
      return fail(c, FAMSEQ_E_HIP, std::string("occupancy query: ") + hipGetErrorString(e));
  }
  c->plan_dirty = false;
  return 0;
}

// What every entry that takes likelihood rows or packed PLs checks first, in the order its callers have come to rely on:
// exactly one of the two (`names`: as the entry calls them), `also` (a complaint of the entry's own about its other
// arguments, or NULL), the device, and n_seq where the entry needs it whichever input is given.
int check_input(famseq_ctx *c, int64_t n_sites, const void *lk, const void *pl16, const char *names, bool need_n_seq, int32_t n_seq,
                const char *also = nullptr) {
  if (n_sites < 0 || (n_sites > 0 && ((lk == nullptr) == (pl16 == nullptr))))
    return fail(c, FAMSEQ_E_ARG, std::string("exactly one of ") + names + " must be given");
  if (also) return fail(c, FAMSEQ_E_ARG, also);
  if (c->device < 0) return fail(c, FAMSEQ_E_NODEVICE, kNoDevice);
  if (need_n_seq && n_seq < 1) return fail(c, FAMSEQ_E_ARG, "n_seq must be >= 1");
  return 0;
}

}  // namespace

extern "C" int famseq_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}


namespace {
famseq_ctx *create_ctx(const Model &model, int device_id, char *err, size_t errlen);
}

extern "C" famseq_ctx *famseq_create(const famseq_model *model, int device_id, char *err, size_t errlen) {
  if (!model) {
    set_err(err, errlen, "model is NULL");
    return nullptr;
  }
  if (model->n_members < 1 || model->n_members > FAMSEQ_MAX_MEMBERS) {
    set_err(err, errlen, "n_members must be 1..20 (famseq_model; famseq_pedigree has no limit)");
    return nullptr;
  }
  return create_ctx(Model(*model), device_id, err, errlen);
}

extern "C" famseq_ctx *famseq_create_pedigree(const famseq_pedigree *pedigree, int device_id, char *err, size_t errlen) {
  if (!pedigree) {
    set_err(err, errlen, "pedigree is NULL");
    return nullptr;
  }
  return create_ctx(Model(*pedigree), device_id, err, errlen);
}

namespace {
famseq_ctx *create_ctx(const Model &model, int device_id, char *err, size_t errlen) {
  famseq_ctx *c = new famseq_ctx;
  c->model = model;
  c->big = model.n_members > FAMSEQ_MAX_MEMBERS;
  try {
    validate_model(c->model);
  } catch (const std::exception &e) {
    set_err(err, errlen, e.what());
    delete c;
    return nullptr;
  }
  if (device_id >= 0) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || device_id >= n) {
      set_err(err, errlen, "no usable HIP device " + std::to_string(device_id) + " (" +
                               (e != hipSuccess ? hipGetErrorString(e) : "device_id out of range") + ")");
      delete c;
      return nullptr;
    }
    hipDeviceProp_t prop;
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) {
      set_err(err, errlen, std::string("hipSetDevice: ") + hipGetErrorString(e));
      delete c;
      return nullptr;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
      set_err(err, errlen, std::string("device is ") + prop.gcnArchName + ", this library only carries gfx950 code");
      delete c;
      return nullptr;
    }
    c->device = device_id;
    c->n_cus = prop.multiProcessorCount;
    for (int s = 0; s < kStages; ++s)
      if ((e = hipStreamCreateWithFlags(&c->stream[s], hipStreamNonBlocking)) != hipSuccess) {
        set_err(err, errlen, std::string("hipStreamCreate: ") + hipGetErrorString(e));
        famseq_destroy(c);
        return nullptr;
      }
    for (int s = 0; s < kSlots; ++s)
      for (hipEvent_t *ev : {&c->ev_in[s], &c->ev_done[s], &c->ev_out[s]})
        if ((e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) {
          set_err(err, errlen, std::string("hipEventCreate: ") + hipGetErrorString(e));
          famseq_destroy(c);
          return nullptr;
        }
  }
  if (refresh_plan(c) != 0) {
    set_err(err, errlen, c->err);
    famseq_destroy(c);
    return nullptr;
  }
  if (c->big) {  // beyond the enumeration's reach: the sum-product engine or nothing
    if (load_or_fail(c, K_ELIM) != 0) {
      set_err(err, errlen, "a pedigree of " + std::to_string(model.n_members) + " members is served by the sum-product engine only: " + c->err);
      famseq_destroy(c);
      return nullptr;
    }
    c->engine = FAMSEQ_ENGINE_ELIM;
  }
  return c;
}
}  // namespace

extern "C" void famseq_destroy(famseq_ctx *c) {
  if (!c) return;
  if (c->device >= 0) {
    (void)hipSetDevice(c->device);
    for (GenKernel &g : c->kern) jit_unload(g.k);
    for (int s = 0; s < kStages; ++s)
      if (c->stream[s]) (void)hipStreamDestroy(c->stream[s]);
    for (int s = 0; s < kSlots; ++s)
      for (hipEvent_t ev : {c->ev_in[s], c->ev_done[s], c->ev_out[s]})
        if (ev) (void)hipEventDestroy(ev);
    if (c->ev_state) (void)hipEventDestroy(c->ev_state);
    for (hipEvent_t ev : c->ev_stage)
      if (ev) (void)hipEventDestroy(ev);
    if (c->stage_mem) (void)hipHostFree(c->stage_mem);
  }
  delete c;  // (its device buffers go with it)
}

extern "C" const char *famseq_last_error(famseq_ctx *c) { return c ? c->err.c_str() : "ctx is NULL"; }

extern "C" int famseq_set_option(famseq_ctx *c, const char *key, int64_t value) {
  if (!c || !key) return FAMSEQ_E_ARG;
  const std::string k(key);
  if (c->big) {  // no enumeration here: its knobs have nothing to act on
    for (const char *e : {"fixed_digits", "low_members", "block_threads", "enum_impl", "group_digits", "pick_lane", "tune", "lane_min_sites", "bulk_min_sites"})
      if (k == e) return fail(c, FAMSEQ_E_ARG, "option " + k + " belongs to the enumeration engine, which serves up to 20 members");
    if (k == "engine" && value == FAMSEQ_ENGINE_ENUM)
      return fail(c, FAMSEQ_E_ARG, "the 3^N enumeration serves up to 20 members; this pedigree has " + std::to_string(c->model.n_members));
    if (k == "call_kernels") return 0;  // (the call path of such a pedigree runs as separate stages)
  }
  // "<stem>_kernels", "<stem>_prior_kernels" of a side product: build (and on a device ctx load) the kernel of that output form now
  for (const SideProduct &p : side_table())
    for (bool site_prior : {false, true})
      if ((!site_prior || p.has_prior()) && k == std::string(p.stem) + (site_prior ? "_prior_kernels" : "_kernels")) {
        if (value < 1 || value > p.n_forms) return fail(c, FAMSEQ_E_ARG, k + " takes " + p.takes);
        return load_or_fail(c, p.kind_of((int)value, site_prior));
      }
  PlanOptions saved = c->opt;
  if (k == "fixed_digits") c->opt.fixed_digits = (int)value;
  else if (k == "low_members") c->opt.low_members = (int)value;
  else if (k == "block_threads") c->opt.block_threads = (int)value;
  else if (k == "grid_blocks") { c->grid_override = value; return 0; }
  else if (k == "enum_impl") {
    if (value < -1 || value > 1) return fail(c, FAMSEQ_E_ARG, "enum_impl must be -1 (auto), 0 (team kernel) or 1 (lane kernel)");
    if (value == 1 && !load_or_remember(c, K_LANE)) return fail(c, FAMSEQ_E_HIP, "lane-per-site kernel unavailable: " + c->kern[K_LANE].error);
    c->enum_impl = (int)value;
    return 0;
  }
  else if (k == "lane_min_sites") { c->lane_min_sites = value; return 0; }
  else if (k == "bulk_min_sites") {  // from how many sites on the bulk slot serves a one-lane-per-site launch; -1: never
    if (value < -1) return fail(c, FAMSEQ_E_ARG, "bulk_min_sites takes a site count, or -1 (the bulk slot is off)");
    c->bulk_min_sites = value;
    return 0;
  }
  else if (k == "tune") {
    if (value != 1) return fail(c, FAMSEQ_E_ARG, "tune takes 1");
    return tune(c);
  }
  else if (k == "pick_lane" || k == "pick_elim") {  // a variant measured elsewhere (the table build() ships): the note tune() would leave
    const bool lane = k == "pick_lane";
    if (value < 0 || value >= (lane ? kEnumVariants : kElimVariants)) return fail(c, FAMSEQ_E_ARG, k + " takes a variant index");
    if (!lane && !elim_supported(c->model, nullptr)) return fail(c, FAMSEQ_E_ARG, "pick_elim: the sum-product engine does not serve this pedigree");
    try {
      jit_write_pick(lane ? enumgen_source(c->model, 0, 0) : elim_source(c->model, 0), (int)value);
    } catch (const std::exception &e) {
      return fail(c, FAMSEQ_E_HIP, e.what());
    }
    if (lane) {  // whatever this context holds of that kernel is dropped; the next use starts from the note
      drop_lane_kernels(c);
    } else {
      c->kern[K_ELIM].drop();
      c->kern[K_PRIOR].drop();  // (it runs in famseq_elim's variant: loaded again, from the note, on its next use)
      if (c->engine == FAMSEQ_ENGINE_ELIM) return load_or_fail(c, K_ELIM);
    }
    return 0;
  }
  else if (k == "prebuild_lane" || k == "prebuild_elim") {  // compile one given variant into the cache (what the tuner will race): no load
    const bool lane = k == "prebuild_lane";
    if (value < 0 || value >= (lane ? kEnumVariants : kElimVariants)) return fail(c, FAMSEQ_E_ARG, k + " takes a variant index");
    try {
      (void)jit_compile(lane ? enumgen_source(c->model, (int)value, 0) : elim_source(c->model, (int)value));
    } catch (const std::exception &e) {
      return fail(c, FAMSEQ_E_HIP, e.what());
    }
    return 0;
  }
  else if (k == "call_kernels") {  // build (and on a device ctx load) the fused call-path forms now rather than on first use
    if (value != 1 && value != 2) return fail(c, FAMSEQ_E_ARG, "call_kernels takes 1 (both forms) or 2 (the form of this ctx's engine)");
    for (int kind : {K_LANE_CALL, K_ELIM_CALL}) {
      if (value == 2 ? kind != (c->engine == FAMSEQ_ENGINE_ELIM ? K_ELIM_CALL : K_LANE_CALL) : kind == K_ELIM_CALL && !elim_supported(c->model, nullptr))
        continue;
      if (!load_or_remember(c, kind)) return fail(c, FAMSEQ_E_HIP, "call-path kernel unavailable: " + c->kern[kind].error);
    }
    return 0;
  }
  else if (k == "prior_kernels") {  // build (and on a device ctx load) the site-prior form of the sum-product kernel now
    if (value != 1) return fail(c, FAMSEQ_E_ARG, "prior_kernels takes 1");
    return load_or_fail(c, K_PRIOR);
  }
  else if (k == "group_digits") {
    if (value < -1 || value > enumgen_max_group_digits(c->model))
      return fail(c, FAMSEQ_E_ARG, "group_digits must be -1 (auto) or 0.." + std::to_string(enumgen_max_group_digits(c->model)) +
                                       " (looped members of this pedigree's enumeration)");
    if (value >= 0 && !load_or_remember(c, K_LANE + (int)value)) return fail(c, FAMSEQ_E_HIP, "lane kernel unavailable: " + c->kern[K_LANE].error);
    c->group_digits = (int)value;
    return 0;
  }
  else if (k == "engine") {
    if (value != FAMSEQ_ENGINE_ENUM && value != FAMSEQ_ENGINE_ELIM) return fail(c, FAMSEQ_E_ARG, "engine must be 0 (enum) or 1 (elim)");
    if (value == FAMSEQ_ENGINE_ELIM) {
      const int rc = load_or_fail(c, K_ELIM);
      if (rc != 0) return rc;
    }
    c->engine = (int)value;
    return 0;
  }
  else if (k == "phase_clock_report") {  // measuring aid: see report_phase_clock
    if (c->device < 0) return fail(c, FAMSEQ_E_NODEVICE, "phase_clock_report needs a device");
    HIP_TRY(c, hipSetDevice(c->device));
    report_phase_clock(c);
    return 0;
  }
  else if (k == "chunk_sites") {
    if (c->device >= 0) HIP_TRY(c, hipSetDevice(c->device));
    c->chunk_sites = value;
    c->slots.release();
    return 0;
  }
  else return fail(c, FAMSEQ_E_ARG, "unknown option " + k);
  c->plan_dirty = true;
  const int rc = refresh_plan(c);
  if (rc != 0) {  // keep the previous, working plan
    c->opt = saved;
    c->plan_dirty = true;
    const std::string why = c->err;
    (void)refresh_plan(c);
    c->err = why;
  }
  return rc;
}

namespace {
std::string json_str(const std::string &v) {  // paths may hold quotes or backslashes
  std::string o;
  for (char ch : v) {
    if (ch == '"' || ch == '\\') o += '\\';
    if ((unsigned char)ch < 0x20) continue;
    o += ch;
  }
  return o;
}
// One form of a side product: "<stem>[_prior]_code_object" and "..._variant" (trio: of the output form asked for last, with every
// form's code object and the number of children beside the plain form's).
std::string side_json(const famseq_ctx *c, const SideProduct &p, bool site_prior) {
  const int form = p.n_forms == 1 ? 1 : site_prior ? c->trio_prior_last : c->trio_last;
  const GenKernel *g = form ? &c->kern[p.kind_of(form, site_prior)] : nullptr;
  const std::string key = std::string(",\"") + p.stem + (site_prior ? "_prior" : "");
  std::string o = key + "_code_object\":\"" + json_str(g ? g->k.path : std::string()) + "\"";
  if (p.n_forms > 1 && !site_prior) {
    o += key + "_code_objects\":[";
    for (int f = 1; f <= p.n_forms; ++f) o += std::string(f > 1 ? "," : "") + "\"" + json_str(c->kern[p.kind_of(f, false)].k.path) + "\"";
    o += "]";
  }
  o += key + "_variant\":" + std::to_string(g ? g->variant : -1);
  if (p.n_forms > 1 && !site_prior) o += key + "_children\":" + std::to_string(trio_children(c->model).size());
  return o;
}
// The side products and K_PRIOR.  The key order is the order they came in: trio and MAP, the site-prior forms of the posterior
// kernel and of those two, then every later product with its site-prior form behind it.
std::string trio_json(const famseq_ctx *c) {
  constexpr int n_first = SIDE_MAP + 1;
  std::string o;
  for (int i = 0; i < n_first; ++i) o += side_json(c, side_table()[i], false);
  o += ",\"prior_code_object\":\"" + json_str(c->kern[K_PRIOR].k.path) + "\",\"prior_variant\":" + std::to_string(c->kern[K_PRIOR].variant);
  for (int i = 0; i < n_first; ++i) o += side_json(c, side_table()[i], true);
  for (int i = n_first; i < SIDE_MUTRATE; ++i)
    o += side_json(c, side_table()[i], false) + (side_table()[i].has_prior() ? side_json(c, side_table()[i], true) : std::string());
  const std::string bt = std::to_string(elim_block_threads(c->model));  // (every side product's kernel runs in these workgroups)
  o += ",\"evidence_block_threads\":" + bt + ",\"loo_block_threads\":" + bt;
  // The products added since stand behind every older key but in front of the mutation-rate profile's four.  That order is kept
  // for one reason only: tests/test_mutrate_host.py pins those four to the end of the plan, and existing tests stay as they are.
  for (int i = SIDE_MUTRATE + 1; i < SIDE_COUNT; ++i)
    o += side_json(c, side_table()[i], false) + (side_table()[i].has_prior() ? side_json(c, side_table()[i], true) : std::string());
  // the mutation rate the origin kernels' allele rows are made for (null: the model's tables are not one rate's)
  char rate[40] = "null";
  double mu = 0;
  if (origin_rate(c->model, &mu)) std::snprintf(rate, sizeof rate, "%.17g", mu);
  o += std::string(",\"origin_mrate\":") + rate;
  return o + side_json(c, side_table()[SIDE_MUTRATE], false) + side_json(c, side_table()[SIDE_MUTRATE], true);
}
}  // namespace

extern "C" const char *famseq_plan_json(famseq_ctx *c) {
  if (!c) return "{}";
  const GenKernel &elim = c->kern[K_ELIM], &lane = c->kern[K_LANE], &elim_call = c->kern[K_ELIM_CALL], &lane_call = c->kern[K_LANE_CALL];
  if (c->big) {
    c->json = "{\"N\":" + std::to_string(c->model.n_members) + ",\"engine\":" + std::to_string(c->engine) + ",\"elim_supported\":1,\"elim_code_object\":\"" +
              json_str(elim.k.path) + "\",\"elim_variant\":" + std::to_string(elim.variant) + ",\"elim_blocks_per_cu\":" +
              std::to_string(elim.blocks_per_cu) + ",\"elim_conditioned_members\":" + std::to_string(elim_conditioned_members(c->model)) +
              ",\"enum_supported\":0,\"device\":" + std::to_string(c->device) + ",\"cus\":" + std::to_string(c->n_cus) + trio_json(c) + "}";
    return c->json.c_str();
  }
  bulk_prebuild(c);  // (a plan-only context: whoever warms a cache through plan() leaves nothing for the first large launch)
  const GenKernel &bulk = c->kern[K_LANE_BULK];
  c->json = c->plan.json();
  c->json.pop_back();
  c->json += ",\"engine\":" + std::to_string(c->engine) + ",\"elim_supported\":" +
             std::string(elim_supported(c->model, nullptr) ? "1" : "0") + ",\"elim_code_object\":\"" + json_str(elim.k.path) +
             "\",\"enum_lane_shape\":\"" + enumgen_describe(c->model, lane.variant) + "\",\"enum_impl\":" + std::to_string(c->enum_impl) + ",\"enum_lane_code_object\":\"" + json_str(lane.k.path) +
             "\",\"enum_lane_failed\":" + std::string(lane.failed ? "1" : "0") + ",\"enum_lane_error\":\"" + json_str(lane.error.substr(0, 400)) + "\"" + ",\"device\":" + std::to_string(c->device) + ",\"cus\":" + std::to_string(c->n_cus) +
             ",\"blocks_per_cu\":" + std::to_string(c->blocks_per_cu) + ",\"elim_variant\":" + std::to_string(elim.variant) +
             ",\"elim_conditioned_members\":" + std::to_string(elim_conditioned_members(c->model)) +
             ",\"elim_blocks_per_cu\":" + std::to_string(elim.blocks_per_cu) + ",\"enum_lane_variant\":" +
             std::to_string(lane.variant) + ",\"enum_lane_blocks_per_cu\":" + std::to_string(lane.blocks_per_cu) +
             ",\"enum_lane_first_variant\":" + std::to_string(lane_first_variant(c)) + ",\"enum_group_digits\":" + std::to_string(c->group_digits) + ",\"enum_group_digits_max\":" +
             std::to_string(enumgen_max_group_digits(c->model)) + ",\"enum_group_digits_last\":" +
             std::to_string(c->last_group_digits) + ",\"enum_group_code_objects\":[";
  for (int d = 1; d <= kEnumMaxGroupDigits; ++d) c->json += std::string(d > 1 ? "," : "") + "\"" + json_str(c->lanes(d).k.path) + "\"";
  c->json += "],\"enum_lane_call_code_object\":\"" + json_str(lane_call.k.path) + "\",\"elim_call_code_object\":\"" +
             json_str(elim_call.k.path) + "\",\"enum_lane_call_error\":\"" + json_str(lane_call.error.substr(0, 300)) + "\",\"elim_call_error\":\"" +
             json_str(elim_call.error.substr(0, 300)) + "\",\"enum_lane_call_reads_rows\":" + std::to_string(c->lane_reads_rows) +
             ",\"enum_lane_call_variant\":" + std::to_string(lane_call.variant) + ",\"elim_call_variant\":" +
             std::to_string(elim_call.variant) + ",\"tune\":\"" +
             json_str(c->tune_report) + "\"" +
             // the bulk slot (kernels.cpp, bulk_serves); the enum_lane_* keys above describe K_LANE whichever kernel served
             // (in front of the side products' keys: the latest of those are pinned to the end of the plan)
             ",\"enum_bulk_code_object\":\"" + json_str(bulk.k.path) + "\",\"enum_bulk_variant\":" + std::to_string(bulk.variant) +
             ",\"enum_bulk_shape\":\"" + (bulk.variant >= 0 ? enumgen_describe(c->model, bulk.variant) : std::string()) +
             "\",\"enum_bulk_min_sites\":" + std::to_string(bulk_min_sites(c)) + ",\"enum_bulk_failed\":" + (bulk.failed ? "1" : "0") +
             ",\"enum_last_kind\":\"" + c->last_kind + "\"" + trio_json(c) + "}";
  return c->json.c_str();
}

extern "C" int famseq_bn_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint8_t *d_flags,
                                      double *d_post, double *d_single, uint8_t *d_status, void *stream) {
  if (!c) return FAMSEQ_E_ARG;
  if (c->device < 0) return fail(c, FAMSEQ_E_NODEVICE, kNoDevice);
  if (n_sites < 0 || (n_sites > 0 && (!d_lk || !d_post))) return fail(c, FAMSEQ_E_ARG, "bad batch arguments");
  if (n_sites == 0) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, launch_engine(c, n_sites, d_lk, d_flags, d_post, d_single, d_status, static_cast<hipStream_t>(stream)));
  return 0;
}

namespace {

// A device-entry call that touches what the context's device entries share (ctx.h, ev_state): begin() puts it behind the last
// such call where that one went to another stream — the event is recorded on that stream only now, behind everything it has
// been given since, so calls that stay on one stream pay nothing — and names its own stream as the one to wait for next.
// Never waits on the host, unless that other stream is gone (destroyed by its owner: the whole device is waited for instead).
struct StateCall {
  hipStream_t stream = nullptr;
  int begin(famseq_ctx *c, hipStream_t s) {
    if (c->state_used && c->state_stream != s) {
      if (!c->ev_state) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_state, hipEventDisableTiming));
      if (hipEventRecord(c->ev_state, c->state_stream) == hipSuccess) {
        HIP_TRY(c, hipStreamWaitEvent(s, c->ev_state, 0));
      } else {
        (void)hipGetLastError();
        HIP_TRY(c, hipDeviceSynchronize());
      }
    }
    c->state_stream = stream = s, c->state_used = true;
    return 0;
  }
};

// Before the host touches that state (a host entry rewrites the maps, the scratch is freed to grow): every device-entry call
// that uses it has run.  (Each is behind its predecessor, so the last one's stream stands for all.)
int state_drained(famseq_ctx *c) {
  if (c->state_used && hipStreamSynchronize(c->state_stream) != hipSuccess) {
    (void)hipGetLastError();
    HIP_TRY(c, hipDeviceSynchronize());
  }
  return 0;
}

// Small host blocks to device memory on `stream`, without waiting for it: through the next pinned slot of the context's ring.
// The host waits only where all kStageRing slots hold copies that have not run yet.
struct StageCopy {
  void *dst;
  const void *src;
  size_t bytes;
};
int stage_copies(famseq_ctx *c, hipStream_t stream, std::initializer_list<StageCopy> list) {
  if (!c->stage_mem) {
    c->stage_bytes = (std::max(sizeof(CallIO), size_t(3) * c->model.n_members * sizeof(int32_t)) + 63) / 64 * 64;
    for (hipEvent_t &ev : c->ev_stage)
      if (!ev) HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    void *p = nullptr;
    HIP_TRY(c, hipHostMalloc(&p, c->stage_bytes * kStageRing, hipHostMallocDefault));
    c->stage_mem = static_cast<char *>(p);
  }
  const int i = c->stage_next;
  if (c->stage_used[i]) HIP_TRY(c, hipEventSynchronize(c->ev_stage[i]));
  char *at = c->stage_mem + size_t(i) * c->stage_bytes;
  size_t used = 0;
  for (const StageCopy &a : list) {
    if (!a.bytes) continue;
    if (used + a.bytes > c->stage_bytes) return fail(c, FAMSEQ_E_HIP, "staging slot too small (internal)");
    std::memcpy(at + used, a.src, a.bytes);
    HIP_TRY(c, hipMemcpyAsync(a.dst, at + used, a.bytes, hipMemcpyHostToDevice, stream));
    used += a.bytes;
  }
  HIP_TRY(c, hipEventRecord(c->ev_stage[i], stream));
  c->stage_used[i] = true;
  c->stage_next = (i + 1) % kStageRing;
  return 0;
}

// Upload the sequenced-member list (VCF column order) and its inverse when it changes.  A host entry (state == NULL) first waits
// for the device-entry calls that read the maps, or that brought them up to date on a stream of the caller's, then copies
// synchronously; a device entry, inside its StateCall, copies on its stream, behind whatever still reads the old maps.
int set_sequenced(famseq_ctx *c, const int32_t *seq, int n_seq, const StateCall *state = nullptr) {
  if (n_seq < 0 || n_seq > c->model.n_members || (n_seq > 0 && !seq)) return fail(c, FAMSEQ_E_ARG, "bad sequenced-member list");
  std::vector<int32_t> v(seq, seq + n_seq), col(c->model.n_members, -1);
  for (int k = 0; k < n_seq; ++k) {
    if (v[k] < 0 || v[k] >= c->model.n_members || col[v[k]] >= 0) return fail(c, FAMSEQ_E_ARG, "bad sequenced-member list");
    col[v[k]] = k;
  }
  if (!state) {
    const int rc = state_drained(c);
    if (rc != 0) return rc;
  }
  if (c->d_seq && v == c->seq_members) return 0;
  for (DevBuf *b : {&c->d_seq, &c->d_col, &c->d_slot})
    if (!*b) HIP_TRY(c, b->alloc(c->model.n_members * sizeof(int32_t)));
  // where a member's printed values go in the call-path kernels' output rows: its column; members without one fill the slots behind
  std::vector<int32_t> slot(col);
  for (int p = 0, next = n_seq; p < c->model.n_members; ++p)
    if (slot[p] < 0) slot[p] = next++;
  const size_t all = slot.size() * sizeof(int32_t);
  if (state) {
    const int rc = stage_copies(c, state->stream, {{c->d_slot.p, slot.data(), all}, {c->d_seq.p, v.data(), n_seq * sizeof(int32_t)}, {c->d_col.p, col.data(), all}});
    if (rc != 0) {
      c->seq_members.assign(1, -1);  // (what reached the device is unknown; no caller can name this list: the next call uploads again)
      return rc;
    }
  } else {
    HIP_TRY(c, hipMemcpy(c->d_slot.p, slot.data(), all, hipMemcpyHostToDevice));
    if (n_seq) HIP_TRY(c, hipMemcpy(c->d_seq.p, v.data(), n_seq * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_col.p, col.data(), all, hipMemcpyHostToDevice));
  }
  c->seq_members = v;
  return 0;
}

bool same_call_io(const CallIO &a, const CallIO &b) {  // (field by field: the struct has padding)
  return a.pl == b.pl && a.lut == b.lut && a.col == b.col && a.slot == b.slot && a.gpp == b.gpp && a.fpp == b.fpp && a.fgt == b.fgt &&
         a.n_seq == b.n_seq && a.magic_w == b.magic_w && a.magic_n == b.magic_n && a.phase_clk == b.phase_clk;
}

}  // namespace

extern "C" int famseq_bn_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint8_t *flags, double *post,
                               double *post_single, uint8_t *status) {
  if (!c) return FAMSEQ_E_ARG;
  if (n_sites < 0 || (n_sites > 0 && (!lk || !post))) return fail(c, FAMSEQ_E_ARG, "bad batch arguments");
  HostIO io;
  io.lk = lk; io.flags = flags; io.post = post; io.single = post_single; io.status = status;
  return run_host(c, n_sites, io, 0);
}

// ---- founder priors per site -----------------------------------------------------------------------------------------

extern "C" void famseq_hwe_priors(int64_t n, const double *af, double *prior) {
  for (int64_t i = 0; i < n; ++i) {
    const double q = af[i], p = 1 - q;
    double *r = prior + 6 * i;
    r[0] = p * p, r[1] = 2 * q * p, r[2] = q * q;
    r[3] = p, r[4] = 0, r[5] = q;
  }
}

namespace {
// What the host entries ask of the prior rows, and the kernel they run.
int prior_ready(famseq_ctx *c, int64_t n_sites, const uint8_t *flags, const double *prior, int kind = K_PRIOR) {
  if (n_sites > 0 && !prior) return fail(c, FAMSEQ_E_ARG, "prior must be given (six doubles per site)");
  if (c->device < 0) return fail(c, FAMSEQ_E_NODEVICE, kNoDevice);
  for (int64_t s = 0; s < n_sites; ++s)  // (the male chrX row is read at chrX sites only)
    for (int k = 0, n = flags && (flags[s] & 2) ? 6 : 3; k < n; ++k)
      if (!(prior[6 * s + k] >= 0 && prior[6 * s + k] <= 1.79769313486231570815e308))
        return fail(c, FAMSEQ_E_ARG, "prior entries must be finite and >= 0 (site " + std::to_string(s) + ")");
  HIP_TRY(c, hipSetDevice(c->device));
  return load_or_fail(c, kind);
}
}  // namespace

extern "C" int famseq_bn_prior_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint8_t *flags, const double *prior,
                                     double *post, double *post_single, uint8_t *status) {
  if (!c) return FAMSEQ_E_ARG;
  if (n_sites < 0 || (n_sites > 0 && (!lk || !post))) return fail(c, FAMSEQ_E_ARG, "bad batch arguments");
  const int rc = prior_ready(c, n_sites, flags, prior);
  if (rc != 0) return rc;
  HostIO io;
  io.lk = lk; io.flags = flags; io.prior = prior; io.post = post; io.single = post_single; io.status = status;
  return run_host(c, n_sites, io, 0);
}

extern "C" int famseq_bn_prior_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint8_t *d_flags,
                                            const double *d_prior, double *d_post, double *d_single, uint8_t *d_status, void *stream) {
  if (!c) return FAMSEQ_E_ARG;
  if (n_sites < 0 || (n_sites > 0 && (!d_lk || !d_post))) return fail(c, FAMSEQ_E_ARG, "bad batch arguments");
  if (n_sites > 0 && !d_prior) return fail(c, FAMSEQ_E_ARG, "d_prior must be given (six doubles per site)");
  if (c->device < 0) return fail(c, FAMSEQ_E_NODEVICE, kNoDevice);
  HIP_TRY(c, hipSetDevice(c->device));
  const int rc = load_or_fail(c, K_PRIOR);
  if (rc != 0 || n_sites == 0) return rc;
  HIP_TRY(c, launch_generated(c, c->kern[K_PRIOR], n_sites, d_lk, d_flags, d_post, d_single, d_status, static_cast<hipStream_t>(stream), 0, {&d_prior}));
  return 0;
}

extern "C" int famseq_bn_batch_sharded(famseq_ctx *const *ctxs, int n_ctx, int64_t n_sites, const double *lk,
                                       const uint8_t *flags, double *post, double *post_single, uint8_t *status) {
  if (!ctxs || n_ctx < 1) return FAMSEQ_E_ARG;
  for (int g = 0; g < n_ctx; ++g)
    if (!ctxs[g] || ctxs[g]->model.n_members != ctxs[0]->model.n_members) return FAMSEQ_E_ARG;
  if (n_sites < 0 || (n_sites > 0 && (!lk || !post))) return fail(ctxs[0], FAMSEQ_E_ARG, "bad batch arguments");
  const int64_t w = int64_t(3) * ctxs[0]->model.n_members;
  std::vector<int> rc(n_ctx, 0);
  std::vector<std::thread> pool;
  for (int g = 0; g < n_ctx; ++g)
    pool.emplace_back([&, g] {
      const int64_t lo = n_sites * g / n_ctx, hi = n_sites * (g + 1) / n_ctx;
      rc[g] = famseq_bn_batch(ctxs[g], hi - lo, lk + lo * w, flags ? flags + lo : nullptr, post + lo * w,
                              post_single ? post_single + lo * w : nullptr, status ? status + lo : nullptr);
    });
  for (std::thread &t : pool) t.join();
  for (int g = 0; g < n_ctx; ++g)
    if (rc[g] != 0) return rc[g];
  return 0;
}

extern "C" int famseq_bn_batch_device_sharded(famseq_ctx *const *ctxs, int n_ctx, const int64_t *n_sites,
                                              const double *const *d_lk, const uint8_t *const *d_flags,
                                              double *const *d_post, double *const *d_single, uint8_t *const *d_status) {
  if (!ctxs || n_ctx < 1 || !n_sites || !d_lk || !d_post) return FAMSEQ_E_ARG;
  for (int g = 0; g < n_ctx; ++g) {
    if (!ctxs[g] || ctxs[g]->model.n_members != ctxs[0]->model.n_members) return FAMSEQ_E_ARG;
    if (ctxs[g]->device < 0) return fail(ctxs[g], FAMSEQ_E_NODEVICE, kNoDevice);
    if (n_sites[g] < 0 || (n_sites[g] > 0 && (!d_lk[g] || !d_post[g]))) return fail(ctxs[g], FAMSEQ_E_ARG, "bad batch arguments");
  }
  std::vector<int> rc(n_ctx, 0);
  std::vector<std::thread> pool;
  for (int g = 0; g < n_ctx; ++g)
    pool.emplace_back([&, g] {
      famseq_ctx *c = ctxs[g];
      rc[g] = [&]() -> int {
        if (n_sites[g] == 0) return 0;
        HIP_TRY(c, hipSetDevice(c->device));  // the device binding is per host thread
        HIP_TRY(c, launch_engine(c, n_sites[g], d_lk[g], d_flags ? d_flags[g] : nullptr, d_post[g],
                                 d_single ? d_single[g] : nullptr, d_status ? d_status[g] : nullptr, c->stream[1]));
        HIP_TRY(c, hipStreamSynchronize(c->stream[1]));
        return 0;
      }();
    });
  for (std::thread &t : pool) t.join();
  for (int g = 0; g < n_ctx; ++g)
    if (rc[g] != 0) return rc[g];
  return 0;
}

extern "C" int famseq_stream_probe(famseq_ctx *c, int64_t n_doubles, const double *d_in, double *d_out1, double *d_out2,
                                   void *stream) {
  if (!c) return FAMSEQ_E_ARG;
  if (c->device < 0) return fail(c, FAMSEQ_E_NODEVICE, kNoDevice);
  if (n_doubles < 0 || (n_doubles > 0 && (!d_in || !d_out1 || !d_out2)) || ((uintptr_t)d_in | (uintptr_t)d_out1 | (uintptr_t)d_out2) & 15)
    return fail(c, FAMSEQ_E_ARG, "bad probe arguments (arrays must be 16-byte aligned)");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, launch_stream_probe(d_in, d_out1, d_out2, n_doubles, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" void *famseq_alloc_pinned(size_t bytes) {
  void *p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}

extern "C" void famseq_free_pinned(void *p) {
  if (p) (void)hipHostFree(p);
}

extern "C" int famseq_bn_call_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16,
                                    const uint8_t *flags, const int32_t *seq_members, int32_t n_seq, double *gpp,
                                    double *fpp, int8_t *fgt, uint8_t *status) {
  if (!c) return FAMSEQ_E_ARG;
  int rc = check_input(c, n_sites, lk, pl16, "lk / pl16", true, n_seq);
  if (rc != 0) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = set_sequenced(c, seq_members, n_seq)) != 0) return rc;
  HostIO io;
  io.lk = lk; io.pl16 = pl16; io.flags = flags; io.gpp = gpp; io.fpp = fpp; io.fgt = fgt; io.status = status;
  return run_host(c, n_sites, io, n_seq);
}

static_assert(kTextStride == FAMSEQ_TEXT_STRIDE, "the header's record size is the text kernel's");

extern "C" int famseq_bn_call_text_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16,
                                         const uint8_t *flags, const int32_t *seq_members, int32_t n_seq, char *text,
                                         uint8_t *status) {
  if (!c) return FAMSEQ_E_ARG;
  int rc = check_input(c, n_sites, lk, pl16, "lk / pl16", true, n_seq, n_sites > 0 && !text ? "text must be given" : nullptr);
  if (rc != 0) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = set_sequenced(c, seq_members, n_seq)) != 0) return rc;
  HostIO io;
  io.lk = lk; io.pl16 = pl16; io.flags = flags; io.text = text; io.status = status;
  return run_host(c, n_sites, io, n_seq);
}

extern "C" int famseq_bn_prior_call_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const uint8_t *flags,
                                          const double *prior, const int32_t *seq_members, int32_t n_seq, double *gpp, double *fpp,
                                          int8_t *fgt, char *text, uint8_t *status) {
  if (!c) return FAMSEQ_E_ARG;
  int rc = check_input(c, n_sites, lk, pl16, "lk / pl16", true, n_seq);
  if (rc != 0 || (rc = prior_ready(c, n_sites, flags, prior)) != 0) return rc;
  if ((rc = set_sequenced(c, seq_members, n_seq)) != 0) return rc;
  HostIO io;
  io.lk = lk; io.pl16 = pl16; io.flags = flags; io.prior = prior; io.status = status;
  if (text) io.text = text;
  else io.gpp = gpp, io.fpp = fpp, io.fgt = fgt;
  return run_host(c, n_sites, io, n_seq);
}

extern "C" int famseq_format_probe(famseq_ctx *c, int64_t n, const double *values, char *out) {
  if (!c) return FAMSEQ_E_ARG;
  if (c->device < 0) return fail(c, FAMSEQ_E_NODEVICE, kNoDevice);
  if (n < 0 || (n > 0 && (!values || !out))) return fail(c, FAMSEQ_E_ARG, "bad probe arguments");
  if (n == 0) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  DevBuf d_in, d_out;
  HIP_TRY(c, d_in.alloc(size_t(n) * sizeof(double)));
  hipError_t e = d_out.alloc(size_t(n) * 16);
  if (e == hipSuccess) e = hipMemcpy(d_in.p, values, size_t(n) * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_g6_probe(d_in.as<double>(), n, d_out.as<char>(), c->stream[1]);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream[1]);
  if (e == hipSuccess) e = hipMemcpy(out, d_out.p, size_t(n) * 16, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(c, FAMSEQ_E_HIP, std::string("famseq_format_probe: ") + hipGetErrorString(e));
  return 0;
}

// The call path on buffers that are resident already (a pipeline that keeps its packed PLs, or its results, in HBM; bench.py's
// `call_path` line): the same kernels as famseq_bn_call_batch, enqueued on the caller's stream, nothing copied.
extern "C" int famseq_bn_call_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                           const uint8_t *d_flags, const int32_t *seq_members, int32_t n_seq, double *d_gpp,
                                           double *d_fpp, int8_t *d_fgt, uint8_t *d_status, char *d_text, void *stream_) {
  if (!c) return FAMSEQ_E_ARG;
  int rc = check_input(c, n_sites, d_lk, d_pl16, "d_lk / d_pl16", true, n_seq);
  if (rc != 0) return rc;
  if (d_text && (reinterpret_cast<uintptr_t>(d_text) & 15)) return fail(c, FAMSEQ_E_ARG, "d_text must be 16-byte aligned");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  // the maps, the argument block and the scratch are the context's: this call takes its place behind the last one that used them
  StateCall state;
  if ((rc = state.begin(c, stream)) != 0 || (rc = set_sequenced(c, seq_members, n_seq, &state)) != 0) return rc;
  if (n_sites == 0) return 0;
  const int N = c->model.n_members;
  const bool want_text = d_text != nullptr;
  // what the stages write: the caller's arrays, or scratch of this context's for those the caller does not ask for but a later
  // stage reads (the text kernel reads all three) or a separate-stages batch passes through (fp64 rows in and out).  Scratch is
  // allocated for what this call needs only: a fused batch with every output given needs none.
  const size_t row = size_t(3) * N * sizeof(double);
  const bool will_fuse = call_fuses(c, n_sites, d_pl16 != nullptr);
  const bool need_rows = !will_fuse, need_called = !will_fuse || (want_text && !(d_gpp && d_fpp && d_fgt)), need_status = !d_status;
  DevBuf *tmp = c->dev_tmp;  // lk, post, single; gpp, fpp, fgt; status
  if ((need_rows && (!tmp[0] || c->dev_tmp_sites < n_sites)) || (need_called && (!tmp[3] || c->dev_tmp_sites < n_sites || c->dev_tmp_seq < n_seq)) ||
      (need_status && (!tmp[6] || c->dev_tmp_sites < n_sites))) {
    // nothing of an earlier call, on whatever stream, may still use what is freed here: the one wait of this entry, on the
    // first call and where a batch is larger than any before
    if ((rc = state_drained(c)) != 0) return rc;
    const int64_t cap = std::max(n_sites, c->dev_tmp_sites);
    const int seqcap = std::max<int>(n_seq, c->dev_tmp_seq);
    const bool had_rows = bool(tmp[0]), had_called = bool(tmp[3]);
    for (int i = 0; i < 7; ++i) tmp[i].release();
    c->dev_tmp_sites = 0;
    if (need_rows || had_rows)
      for (int i = 0; i < 3; ++i) HIP_TRY(c, tmp[i].alloc(size_t(cap) * row));
    if (need_called || had_called) {
      for (int i = 3; i < 5; ++i) HIP_TRY(c, tmp[i].alloc(size_t(cap) * 3 * seqcap * sizeof(double)));
      HIP_TRY(c, tmp[5].alloc(size_t(cap) * seqcap));
    }
    HIP_TRY(c, tmp[6].alloc(size_t(cap)));
    c->dev_tmp_sites = cap, c->dev_tmp_seq = seqcap;
  }
  double *const t_lk = tmp[0].as<double>(), *const t_post = tmp[1].as<double>(), *const t_single = tmp[2].as<double>();
  double *const t_gpp = tmp[3].as<double>(), *const t_fpp = tmp[4].as<double>();
  int8_t *const t_fgt = tmp[5].as<int8_t>();
  double *gpp = d_gpp ? d_gpp : (want_text ? t_gpp : nullptr), *fpp = d_fpp ? d_fpp : (want_text ? t_fpp : nullptr);
  int8_t *fgt = d_fgt ? d_fgt : (want_text ? t_fgt : nullptr);
  uint8_t *status = d_status ? d_status : tmp[6].as<uint8_t>();
  if (d_pl16 && (rc = upload_lut(c)) != 0) return rc;
  const CallIO cio = make_call_io(c, d_pl16, gpp, fpp, fgt, n_seq);
  if (!c->d_call_dev) HIP_TRY(c, c->d_call_dev.alloc(sizeof(CallIO)));
  if (!c->call_dev_valid || !same_call_io(cio, c->call_dev_host)) {
    // the argument block changes only when the caller's pointers do: written on this stream, behind whatever may still read
    // the old one (an earlier call on another stream: StateCall)
    c->call_dev_valid = false;
    if ((rc = stage_copies(c, stream, {{c->d_call_dev.p, &cio, sizeof cio}})) != 0) return rc;
    c->call_dev_host = cio, c->call_dev_valid = true;
  }
  hipError_t e = hipSuccess;
  const bool fused = launch_engine_fused(c, n_sites, d_lk, d_flags, status, d_pl16 != nullptr, c->d_call_dev.as<CallIO>(), stream, &e);
  if (fused) HIP_TRY(c, e);
  if (!fused) {
    if (!t_lk || !t_gpp) return fail(c, FAMSEQ_E_HIP, "call path: the batch left the fused kernel without scratch rows (internal)");
    const double *lk = d_lk;
    if (d_pl16) {
      HIP_TRY(c, launch_unpack_pl16(d_pl16, c->d_col.as<int32_t>(), c->d_lut.as<double>(), N, n_seq, n_sites, t_lk, stream));
      lk = t_lk;
    }
    HIP_TRY(c, launch_engine(c, n_sites, lk, d_flags, t_post, t_single, status, stream));
    HIP_TRY(c, launch_phred_call(t_post, t_single, status, c->d_seq.as<int32_t>(), N, n_seq, n_sites, gpp ? gpp : t_gpp, fpp ? fpp : t_fpp,
                                 fgt ? fgt : t_fgt, stream));
  }
  if (want_text) HIP_TRY(c, launch_text_call(gpp ? gpp : t_gpp, fpp ? fpp : t_fpp, fgt ? fgt : t_fgt, n_sites * n_seq, d_text, stream));
  return 0;
}

// ---- trio posteriors -------------------------------------------------------------------------------------------------

extern "C" int famseq_trio_children(famseq_ctx *c, int32_t *idx) {
  if (!c) return FAMSEQ_E_ARG;
  std::string why;
  if (!elim_supported(c->model, &why)) return fail(c, FAMSEQ_E_ARG, "trio posteriors (sum-product engine): " + why);
  const std::vector<int> kids = trio_children(c->model);
  if (idx) std::copy(kids.begin(), kids.end(), idx);
  return (int)kids.size();
}

namespace {

int trio_form(const void *joint, const void *dnm) { return (joint ? 2 : 0) | (dnm || !joint ? 1 : 0); }

// Arguments the side products' entries check the same way; loads the kernel of that kind (trio: of the form the outputs ask for).
// state: a device entry's (on `stream`), begun here where the input is packed — the maps and the unpacked rows are the
// context's; on likelihood rows a device entry uses nothing of the context's that changes.  NULL: a host entry.
int trio_prologue(famseq_ctx *c, int64_t n_sites, const void *lk, const void *pl16, const int32_t *seq_members, int32_t n_seq,
                  int kind, StateCall *state = nullptr, hipStream_t stream = nullptr) {
  int rc = check_input(c, n_sites, lk, pl16, "lk / pl16", false, n_seq);
  if (rc != 0) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = load_or_fail(c, kind)) != 0) return rc;
  if (pl16) {
    if (n_seq < 1) return fail(c, FAMSEQ_E_ARG, "n_seq must be >= 1");
    if (state && (rc = state->begin(c, stream)) != 0) return rc;
    if ((rc = set_sequenced(c, seq_members, n_seq, state)) != 0) return rc;
    if ((rc = upload_lut(c)) != 0) return rc;
  }
  return 0;
}

// What the side products' entries below share.  On the device path (`device`) the arrays are the caller's resident buffers and the
// kernel is enqueued on `stream`; on the host path they are chunked and pipelined (side_batch) on the product's own buffers.
// The order of the checks is what callers have come to rely on: the product's extra arguments (check_extra), then a site-prior
// device entry asks for d_prior, a site-prior host entry checks its input and its prior rows (prior_ready), then every entry
// trio_prologue.
struct SideIn {
  int64_t n_sites;
  const double *lk;
  const uint16_t *pl16;
  const int32_t *seq_members;
  int32_t n_seq;
  const uint8_t *flags;
  const double *prior = nullptr;  // the site-prior entries' rows
};
struct SideOut {
  void *a, *b;  // the product's two outputs per site
  uint8_t *status;
  void *stream = nullptr;  // the device entries' hipStream_t
};

// What a product's ExtraSpec asks of the entry's extra arguments.  Said before anything else, so that a context without a device
// says it too.  A device entry's table is resident: given or not is all that can be said of it.
int check_extra(famseq_ctx *c, const ExtraSpec &xs, const SideExtra &x, int64_t n_sites, bool device) {
  if (xs.precondition && xs.precondition(c) != 0) return FAMSEQ_E_ARG;
  if (xs.count && (x.count < xs.lo || x.count > xs.hi))
    return fail(c, FAMSEQ_E_ARG, std::string(xs.count) + " must be " + std::to_string(xs.lo) + ".." + std::to_string(xs.hi) + ", got " +
                                     std::to_string(x.count));
  if (std::strchr(xs.params, 'b') && x.site_base < 0) return fail(c, FAMSEQ_E_ARG, "site_base must be >= 0, got " + std::to_string(x.site_base));
  if (xs.name && !x.table)
    return fail(c, FAMSEQ_E_ARG, std::string(device && xs.device_name ? xs.device_name : xs.name) + " must be given (" +
                                     (device && xs.device_given ? xs.device_given : xs.given) + ")");
  return !device && xs.check ? xs.check(c, x.table, x.count, n_sites) : 0;
}

// The device table of a product that keeps one (ExtraSpec::via X_CALL: a host entry's table; X_CONST: the product's constant), in
// *d_table.  The buffer is allocated once, at the largest count.  X_CALL: the table goes through the copy the context keeps, on
// the stream the chunks' kernels run on: ordered with them by the stream itself, and the copy outlives the call's arrays.  (A
// host entry returns with its streams drained, so neither is in use by an earlier call.)  X_CONST: uploaded on its first use.
int stage_extra(famseq_ctx *c, SideId id, const ExtraSpec &xs, const SideExtra &x, const void **d_table) {
  DevBuf &d = c->d_extra[id];
  const bool once = xs.via == X_CONST;
  if (!once || !d) {
    const size_t bytes = xs.bytes(c->model) * x.count;
    if (!d) HIP_TRY(c, d.alloc(xs.bytes(c->model) * xs.hi));
    std::vector<uint8_t> &h = c->extra_host[id];
    h.resize(bytes);
    if (xs.build) xs.build(c, x.table, x.count, h.data());
    else std::memcpy(h.data(), x.table, bytes);
    if (!once) HIP_TRY(c, hipMemcpyAsync(d.p, h.data(), bytes, hipMemcpyHostToDevice, c->stream[1]));
    else if (const hipError_t e = hipMemcpy(d.p, h.data(), bytes, hipMemcpyHostToDevice); e != hipSuccess) {  // (blocking: done when it returns)
      d.release();
      HIP_TRY(c, e);
    }
  }
  *d_table = d.p;
  return 0;
}

int side_entry(famseq_ctx *c, SideId id, int form, bool site_prior, bool device, const SideIn &in, const SideOut &out, const SideExtra &x = {}) {
  if (!c) return FAMSEQ_E_ARG;
  const SideProduct &p = side_table()[id];
  const ExtraSpec &xs = p.extra;
  if (check_extra(c, xs, x, in.n_sites, device) != 0) return FAMSEQ_E_ARG;
  const int kind = p.kind_of(form, site_prior);
  const int64_t n_sites = in.n_sites;
  const double *prior = in.prior;
  int rc;
  if (site_prior && device) {
    if (n_sites > 0 && !prior) return fail(c, FAMSEQ_E_ARG, "d_prior must be given (six doubles per site)");
  } else if (site_prior) {
    if ((rc = check_input(c, n_sites, in.lk, in.pl16, "lk / pl16", false, in.n_seq)) != 0 || (rc = prior_ready(c, n_sites, in.flags, prior, kind)) != 0)
      return rc;
  }
  hipStream_t stream = static_cast<hipStream_t>(out.stream);
  StateCall state;  // (a device entry on packed input)
  if ((rc = trio_prologue(c, n_sites, in.lk, in.pl16, in.seq_members, in.n_seq, kind, device ? &state : nullptr, stream)) != 0 || n_sites == 0)
    return rc;
  // the kernel's arguments in front of the prior rows, in the order the product's row gives
  const void *table = x.table;
  if ((xs.via == X_CONST || (xs.via == X_CALL && !device)) && (rc = stage_extra(c, id, xs, x, &table)) != 0) return rc;
  const int32_t count = x.count;
  const unsigned long seed = (unsigned long)x.seed;
  const long site_base = long(x.site_base);
  MoreArgs lead;
  PerChunk per{prior, 6 * sizeof(double)};  // (the host path)
  for (const char *a = xs.params; *a; ++a) switch (*a) {
      case 't':
        if (xs.via == X_SITE) per = {x.table, xs.bytes(c->model), lead.n};  // (the chunk's staged copy)
        lead.add(&table);
        break;
      case 'n': lead.add(&count); break;
      case 's': lead.add(&seed); break;
      case 'b':
        per.base_at = lead.n, per.site_base = x.site_base;
        lead.add(&site_base);
        break;
    }
  if (!device) {
    size_t row[2];
    p.rows(c->model, count, row);
    return side_batch(c, c->side_slots[id], c->kern[kind], n_sites, in.lk, in.pl16, in.n_seq, in.flags, out.a, row[0], out.b, row[1], out.status, lead,
                      per);
  }
  const double *d_lk = in.lk;
  if (in.pl16) {  // packed input is unpacked into likelihood rows this context keeps (grown on demand)
    const int N = c->model.n_members;
    if (c->trio_dev_sites < n_sites) {
      if ((rc = state_drained(c)) != 0) return rc;  // nothing of an earlier call, on whatever stream, may still use what is freed here
      c->trio_dev_sites = 0;
      HIP_TRY(c, c->trio_dev_lk.alloc(size_t(n_sites) * 3 * N * sizeof(double)));
      c->trio_dev_sites = n_sites;
    }
    d_lk = c->trio_dev_lk.as<double>();
    HIP_TRY(c, launch_unpack_pl16(in.pl16, c->d_col.as<int32_t>(), c->d_lut.as<double>(), N, in.n_seq, n_sites, c->trio_dev_lk.as<double>(), stream));
  }
  lead.add(&prior);  // (behind the last parameter of a plain form: not read)
  HIP_TRY(c, launch_generated(c, c->kern[kind], n_sites, d_lk, in.flags, out.a, out.b, out.status, stream, 0, lead));
  return 0;
}

}  // namespace

// ---- the side products (the rows of side_table()), each plain and with the founders' prior per site, on host and on resident
// ---- buffers: one call of side_entry with the common arguments, the outputs and what the product takes beside ------------------

extern "C" int famseq_trio_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                 int32_t n_seq, const uint8_t *flags, double *joint, double *dnm, uint8_t *status) {
  return side_entry(c, SIDE_TRIO, trio_form(joint, dnm), false, false, {n_sites, lk, pl16, seq_members, n_seq, flags}, {joint, dnm, status});
}

extern "C" int famseq_trio_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                        const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, double *d_joint,
                                        double *d_dnm, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_TRIO, trio_form(d_joint, d_dnm), false, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags},
                    {d_joint, d_dnm, d_status, stream});
}

extern "C" int famseq_trio_prior_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                       int32_t n_seq, const uint8_t *flags, const double *prior, double *joint, double *dnm,
                                       uint8_t *status) {
  return side_entry(c, SIDE_TRIO, trio_form(joint, dnm), true, false, {n_sites, lk, pl16, seq_members, n_seq, flags, prior}, {joint, dnm, status});
}

extern "C" int famseq_trio_prior_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                              const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                              double *d_joint, double *d_dnm, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_TRIO, trio_form(d_joint, d_dnm), true, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags, d_prior},
                    {d_joint, d_dnm, d_status, stream});
}

extern "C" int famseq_map_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                int32_t n_seq, const uint8_t *flags, int8_t *map_gt, double *map_post, uint8_t *status) {
  return side_entry(c, SIDE_MAP, 1, false, false, {n_sites, lk, pl16, seq_members, n_seq, flags}, {map_gt, map_post, status});
}

extern "C" int famseq_map_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                       const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, int8_t *d_map_gt,
                                       double *d_map_post, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_MAP, 1, false, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags}, {d_map_gt, d_map_post, d_status, stream});
}

extern "C" int famseq_map_prior_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                      int32_t n_seq, const uint8_t *flags, const double *prior, int8_t *map_gt, double *map_post,
                                      uint8_t *status) {
  return side_entry(c, SIDE_MAP, 1, true, false, {n_sites, lk, pl16, seq_members, n_seq, flags, prior}, {map_gt, map_post, status});
}

extern "C" int famseq_map_prior_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                             const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                             int8_t *d_map_gt, double *d_map_post, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_MAP, 1, true, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags, d_prior},
                    {d_map_gt, d_map_post, d_status, stream});
}

extern "C" int famseq_evidence_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                     int32_t n_seq, const uint8_t *flags, double *loglik, double *pref, uint8_t *status) {
  return side_entry(c, SIDE_EVID, 1, false, false, {n_sites, lk, pl16, seq_members, n_seq, flags}, {loglik, pref, status});
}

extern "C" int famseq_evidence_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                            const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, double *d_loglik,
                                            double *d_pref, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_EVID, 1, false, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags}, {d_loglik, d_pref, d_status, stream});
}

extern "C" int famseq_evidence_prior_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16,
                                           const int32_t *seq_members, int32_t n_seq, const uint8_t *flags, const double *prior,
                                           double *loglik, double *pref, uint8_t *status) {
  return side_entry(c, SIDE_EVID, 1, true, false, {n_sites, lk, pl16, seq_members, n_seq, flags, prior}, {loglik, pref, status});
}

extern "C" int famseq_evidence_prior_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                                  const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                                  double *d_loglik, double *d_pref, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_EVID, 1, true, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags, d_prior}, {d_loglik, d_pref, d_status, stream});
}

extern "C" int famseq_loo_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                int32_t n_seq, const uint8_t *flags, double *loo, double *fit, uint8_t *status) {
  return side_entry(c, SIDE_LOO, 1, false, false, {n_sites, lk, pl16, seq_members, n_seq, flags}, {loo, fit, status});
}

extern "C" int famseq_loo_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                       const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, double *d_loo, double *d_fit,
                                       uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_LOO, 1, false, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags}, {d_loo, d_fit, d_status, stream});
}

extern "C" int famseq_loo_prior_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                      int32_t n_seq, const uint8_t *flags, const double *prior, double *loo, double *fit, uint8_t *status) {
  return side_entry(c, SIDE_LOO, 1, true, false, {n_sites, lk, pl16, seq_members, n_seq, flags, prior}, {loo, fit, status});
}

extern "C" int famseq_loo_prior_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                             const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                             double *d_loo, double *d_fit, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_LOO, 1, true, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags, d_prior}, {d_loo, d_fit, d_status, stream});
}

extern "C" int famseq_pattern_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                    int32_t n_seq, const uint8_t *flags, const uint8_t *masks, int32_t n_patterns, double *pat_post,
                                    double *loglik, uint8_t *status) {
  return side_entry(c, SIDE_PATTERN, 1, false, false, {n_sites, lk, pl16, seq_members, n_seq, flags},
                    {pat_post, loglik, status}, {masks, n_patterns});
}

extern "C" int famseq_pattern_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                           const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const uint8_t *d_masks,
                                           int32_t n_patterns, double *d_pat_post, double *d_loglik, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_PATTERN, 1, false, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags},
                    {d_pat_post, d_loglik, d_status, stream}, {d_masks, n_patterns});
}

extern "C" int famseq_pattern_prior_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16,
                                          const int32_t *seq_members, int32_t n_seq, const uint8_t *flags, const double *prior,
                                          const uint8_t *masks, int32_t n_patterns, double *pat_post, double *loglik, uint8_t *status) {
  return side_entry(c, SIDE_PATTERN, 1, true, false, {n_sites, lk, pl16, seq_members, n_seq, flags, prior},
                    {pat_post, loglik, status}, {masks, n_patterns});
}

extern "C" int famseq_pattern_prior_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                                 const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                                 const uint8_t *d_masks, int32_t n_patterns, double *d_pat_post, double *d_loglik,
                                                 uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_PATTERN, 1, true, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags, d_prior},
                    {d_pat_post, d_loglik, d_status, stream}, {d_masks, n_patterns});
}

// ---- exact joint posterior draws: the MAP entries with the seed, the first site's absolute index and the draws per site -------

extern "C" int famseq_sample_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                   int32_t n_seq, const uint8_t *flags, uint64_t seed, int64_t site_base, int32_t n_draws, int8_t *samp_gt,
                                   double *samp_post, uint8_t *status) {
  return side_entry(c, SIDE_SAMPLE, 1, false, false, {n_sites, lk, pl16, seq_members, n_seq, flags},
                    {samp_gt, samp_post, status}, {seed, site_base, n_draws});
}

extern "C" int famseq_sample_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                          const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, uint64_t seed, int64_t site_base,
                                          int32_t n_draws, int8_t *d_samp_gt, double *d_samp_post, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_SAMPLE, 1, false, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags},
                    {d_samp_gt, d_samp_post, d_status, stream}, {seed, site_base, n_draws});
}

extern "C" int famseq_sample_prior_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                         int32_t n_seq, const uint8_t *flags, const double *prior, uint64_t seed, int64_t site_base,
                                         int32_t n_draws, int8_t *samp_gt, double *samp_post, uint8_t *status) {
  return side_entry(c, SIDE_SAMPLE, 1, true, false, {n_sites, lk, pl16, seq_members, n_seq, flags, prior},
                    {samp_gt, samp_post, status}, {seed, site_base, n_draws});
}

extern "C" int famseq_sample_prior_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                                const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                                uint64_t seed, int64_t site_base, int32_t n_draws, int8_t *d_samp_gt, double *d_samp_post,
                                                uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_SAMPLE, 1, true, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags, d_prior},
                    {d_samp_gt, d_samp_post, d_status, stream}, {seed, site_base, n_draws});
}

// ---- the founders' allele frequency by maximum likelihood: the evidence entries with the start values and the number of steps ---

extern "C" int famseq_af_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                               int32_t n_seq, const uint8_t *flags, const double *af0, int32_t n_iter, double *af, double *loglik,
                               uint8_t *status) {
  return side_entry(c, SIDE_AF, 1, false, false, {n_sites, lk, pl16, seq_members, n_seq, flags}, {af, loglik, status}, {af0, n_iter});
}

extern "C" int famseq_af_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16, const int32_t *seq_members,
                                      int32_t n_seq, const uint8_t *d_flags, const double *d_af0, int32_t n_iter, double *d_af,
                                      double *d_loglik, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_AF, 1, false, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags},
                    {d_af, d_loglik, d_status, stream}, {d_af0, n_iter});
}

// ---- relabelling evidence: the evidence entries with the assignments of rows to members and their number -------------------

extern "C" int famseq_relabel_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                    int32_t n_seq, const uint8_t *flags, const int32_t *assign, int32_t n_assign, double *alt_loglik,
                                    double *loglik, uint8_t *status) {
  return side_entry(c, SIDE_RELABEL, 1, false, false, {n_sites, lk, pl16, seq_members, n_seq, flags},
                    {alt_loglik, loglik, status}, {assign, n_assign});
}

extern "C" int famseq_relabel_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                           const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const int32_t *d_assign,
                                           int32_t n_assign, double *d_alt_loglik, double *d_loglik, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_RELABEL, 1, false, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags},
                    {d_alt_loglik, d_loglik, d_status, stream}, {d_assign, n_assign});
}

extern "C" int famseq_relabel_prior_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16,
                                          const int32_t *seq_members, int32_t n_seq, const uint8_t *flags, const double *prior,
                                          const int32_t *assign, int32_t n_assign, double *alt_loglik, double *loglik, uint8_t *status) {
  return side_entry(c, SIDE_RELABEL, 1, true, false, {n_sites, lk, pl16, seq_members, n_seq, flags, prior},
                    {alt_loglik, loglik, status}, {assign, n_assign});
}

extern "C" int famseq_relabel_prior_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                                 const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                                 const int32_t *d_assign, int32_t n_assign, double *d_alt_loglik, double *d_loglik,
                                                 uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_RELABEL, 1, true, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags, d_prior},
                    {d_alt_loglik, d_loglik, d_status, stream}, {d_assign, n_assign});
}

// ---- the mutation-rate likelihood profile: the evidence entries with one factor table per rate ----------------------------------

extern "C" int famseq_rate_tables(famseq_ctx *c, const double *rates, int32_t n_rates, double *tables) {
  if (!c) return FAMSEQ_E_ARG;
  if (check_extra(c, side_table()[SIDE_MUTRATE].extra, {rates, n_rates}, 0, false) != 0) return FAMSEQ_E_ARG;
  if (!tables) return fail(c, FAMSEQ_E_ARG, "tables must be given (n_rates blocks of " + std::to_string(FAMSEQ_RATE_TABLE_DOUBLES) + " doubles)");
  rate_tables(c->model, rates, n_rates, tables);
  return 0;
}

extern "C" int famseq_mutrate_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                    int32_t n_seq, const uint8_t *flags, const double *rates, int32_t n_rates, double *rate_loglik,
                                    double *loglik, uint8_t *status) {
  return side_entry(c, SIDE_MUTRATE, 1, false, false, {n_sites, lk, pl16, seq_members, n_seq, flags},
                    {rate_loglik, loglik, status}, {rates, n_rates});
}

extern "C" int famseq_mutrate_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                           const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_tables,
                                           int32_t n_rates, double *d_rate_loglik, double *d_loglik, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_MUTRATE, 1, false, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags},
                    {d_rate_loglik, d_loglik, d_status, stream}, {d_tables, n_rates});
}

extern "C" int famseq_mutrate_prior_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16,
                                          const int32_t *seq_members, int32_t n_seq, const uint8_t *flags, const double *prior,
                                          const double *rates, int32_t n_rates, double *rate_loglik, double *loglik, uint8_t *status) {
  return side_entry(c, SIDE_MUTRATE, 1, true, false, {n_sites, lk, pl16, seq_members, n_seq, flags, prior},
                    {rate_loglik, loglik, status}, {rates, n_rates});
}

extern "C" int famseq_mutrate_prior_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                                 const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                                 const double *d_tables, int32_t n_rates, double *d_rate_loglik, double *d_loglik,
                                                 uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_MUTRATE, 1, true, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags, d_prior},
                    {d_rate_loglik, d_loglik, d_status, stream}, {d_tables, n_rates});
}

// ---- phase by transmission: each child's alleles by parent of origin, and the transmissions from heterozygous parents ----------

extern "C" int famseq_allele_tables(famseq_ctx *c, double *tables) {
  if (!c) return FAMSEQ_E_ARG;
  if (origin_model(c) != 0) return FAMSEQ_E_ARG;
  if (!tables) return fail(c, FAMSEQ_E_ARG, "tables must be given (" + std::to_string(FAMSEQ_ALLELE_TABLE_DOUBLES) + " doubles)");
  build_allele_tables(c->origin_mrate, tables);
  return 0;
}

extern "C" int famseq_origin_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                   int32_t n_seq, const uint8_t *flags, double *origin, double *hettx, uint8_t *status) {
  return side_entry(c, SIDE_ORIGIN, 1, false, false, {n_sites, lk, pl16, seq_members, n_seq, flags}, {origin, hettx, status});
}

extern "C" int famseq_origin_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                          const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, double *d_origin,
                                          double *d_hettx, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_ORIGIN, 1, false, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags}, {d_origin, d_hettx, d_status, stream});
}

extern "C" int famseq_origin_prior_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                         int32_t n_seq, const uint8_t *flags, const double *prior, double *origin, double *hettx,
                                         uint8_t *status) {
  return side_entry(c, SIDE_ORIGIN, 1, true, false, {n_sites, lk, pl16, seq_members, n_seq, flags, prior}, {origin, hettx, status});
}

extern "C" int famseq_origin_prior_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                                const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                                double *d_origin, double *d_hettx, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_ORIGIN, 1, true, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags, d_prior},
                    {d_origin, d_hettx, d_status, stream});
}

// ---- per-member genotype weights: the evidence entries with one table of weights per pass --------------------------------------

extern "C" int famseq_weight_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                   int32_t n_seq, const uint8_t *flags, const double *weights, int32_t n_weights, double *wt_loglik,
                                   double *loglik, uint8_t *status) {
  return side_entry(c, SIDE_WEIGHT, 1, false, false, {n_sites, lk, pl16, seq_members, n_seq, flags},
                    {wt_loglik, loglik, status}, {weights, n_weights});
}

extern "C" int famseq_weight_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                          const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_weights,
                                          int32_t n_weights, double *d_wt_loglik, double *d_loglik, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_WEIGHT, 1, false, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags},
                    {d_wt_loglik, d_loglik, d_status, stream}, {d_weights, n_weights});
}

extern "C" int famseq_weight_prior_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16,
                                         const int32_t *seq_members, int32_t n_seq, const uint8_t *flags, const double *prior,
                                         const double *weights, int32_t n_weights, double *wt_loglik, double *loglik, uint8_t *status) {
  return side_entry(c, SIDE_WEIGHT, 1, true, false, {n_sites, lk, pl16, seq_members, n_seq, flags, prior},
                    {wt_loglik, loglik, status}, {weights, n_weights});
}

extern "C" int famseq_weight_prior_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                                const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                                const double *d_weights, int32_t n_weights, double *d_wt_loglik, double *d_loglik,
                                                uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_WEIGHT, 1, true, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags, d_prior},
                    {d_wt_loglik, d_loglik, d_status, stream}, {d_weights, n_weights});
}

// ---- complex per-member weights: the weight entries with complex tables, two doubles out per table and site ---------------------

extern "C" int famseq_charfn_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                   int32_t n_seq, const uint8_t *flags, const double *cweights, int32_t n_tables, double *cf,
                                   double *loglik, uint8_t *status) {
  return side_entry(c, SIDE_CHARFN, 1, false, false, {n_sites, lk, pl16, seq_members, n_seq, flags},
                    {cf, loglik, status}, {cweights, n_tables});
}

extern "C" int famseq_charfn_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                          const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_cweights,
                                          int32_t n_tables, double *d_cf, double *d_loglik, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_CHARFN, 1, false, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags},
                    {d_cf, d_loglik, d_status, stream}, {d_cweights, n_tables});
}

extern "C" int famseq_charfn_prior_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16,
                                         const int32_t *seq_members, int32_t n_seq, const uint8_t *flags, const double *prior,
                                         const double *cweights, int32_t n_tables, double *cf, double *loglik, uint8_t *status) {
  return side_entry(c, SIDE_CHARFN, 1, true, false, {n_sites, lk, pl16, seq_members, n_seq, flags, prior},
                    {cf, loglik, status}, {cweights, n_tables});
}

extern "C" int famseq_charfn_prior_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                                const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                                const double *d_cweights, int32_t n_tables, double *d_cf, double *d_loglik,
                                                uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_CHARFN, 1, true, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags, d_prior},
                    {d_cf, d_loglik, d_status, stream}, {d_cweights, n_tables});
}

// ---- max-marginals and the runner-up of the joint call: the MAP entries with a row per member in the place of one genotype ------

extern "C" int famseq_maxmarg_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                    int32_t n_seq, const uint8_t *flags, double *maxmarg, double *top, uint8_t *status) {
  return side_entry(c, SIDE_MAXMARG, 1, false, false, {n_sites, lk, pl16, seq_members, n_seq, flags}, {maxmarg, top, status});
}

extern "C" int famseq_maxmarg_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                           const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, double *d_maxmarg, double *d_top,
                                           uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_MAXMARG, 1, false, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags}, {d_maxmarg, d_top, d_status, stream});
}

extern "C" int famseq_maxmarg_prior_batch(famseq_ctx *c, int64_t n_sites, const double *lk, const uint16_t *pl16, const int32_t *seq_members,
                                          int32_t n_seq, const uint8_t *flags, const double *prior, double *maxmarg, double *top, uint8_t *status) {
  return side_entry(c, SIDE_MAXMARG, 1, true, false, {n_sites, lk, pl16, seq_members, n_seq, flags, prior}, {maxmarg, top, status});
}

extern "C" int famseq_maxmarg_prior_batch_device(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint16_t *d_pl16,
                                                 const int32_t *seq_members, int32_t n_seq, const uint8_t *d_flags, const double *d_prior,
                                                 double *d_maxmarg, double *d_top, uint8_t *d_status, void *stream) {
  return side_entry(c, SIDE_MAXMARG, 1, true, true, {n_sites, d_lk, d_pl16, seq_members, n_seq, d_flags, d_prior},
                    {d_maxmarg, d_top, d_status, stream});
}

// The sampling kernels' generator on the host: the text they carry (philox_src.h), compiled here.
namespace {
#define FS_PHILOX_FN inline
#define FS_PHILOX_DEF(...) __VA_ARGS__
#include "philox_src.h"
#undef FS_PHILOX_DEF
#undef FS_PHILOX_FN
}  // namespace

extern "C" void famseq_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  unsigned o[4];
  fs_philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], o);
  for (int i = 0; i < 4; ++i) out[i] = o[i];
}
