// tex_kat.hip -- the RT path's texture sampler (gfx::tex_read, which
// dispatches to tex_read_fmt<FMT>, and the generic gfx::tex_read_any: the
// functions every shaded ray of rt_kernel / pt_kernel / rt_om calls) over a
// table of sample records, for known-answer tests against the independent
// model (tests/tex_reference.py, tests/test_gpu_tex_unit.py).  A record holds
// the sampler state a drawcall record would (any wrapu / wrapv pair, any
// format x filter: states a scene cannot express) and one coordinate pair.
// Thread per record.
#include <hip/hip_runtime.h>

#include "gfx_device.h"

typedef struct {
  uint32_t tex_off;               // device address of the level's texels (below 4 GiB)
  uint32_t logw, logh, format, filter, wrapu, wrapv, stride;
  int32_t u, v;                   // TFixed<23>
} tex_kat_rec_t;

typedef struct {
  uint64_t rec_addr;   // tex_kat_rec_t [count]
  uint64_t out_addr;   // uint32 [count * 2]: tex_read, tex_read_any
  uint32_t count;
  uint32_t pad;
} tex_kat_arg_t;

static __device__ __forceinline__ void kernel_body(const vx_task_t& task, tex_kat_arg_t* a) {
  const uint32_t i = task.task_id;
  const tex_kat_rec_t r = vx_ptr<tex_kat_rec_t>(a->rec_addr)[i];
  const vx_arena A = vx_arena::get();
  gfx::DcState s;
  s.flags = 0;
  s.logw = r.logw; s.logh = r.logh; s.format = r.format; s.filter = r.filter;
  s.wrapu = r.wrapu; s.wrapv = r.wrapv; s.stride = r.stride; s.tex_off = r.tex_off;
  uint32_t* out = vx_ptr<uint32_t>(a->out_addr);
  out[2 * i] = gfx::tex_read(A, s, r.u, r.v);
  out[2 * i + 1] = gfx::tex_read_any(A, s, r.u, r.v);
}

VX_MAIN(tex_kat_arg_t, arg, 256) {
  return vx_spawn_tasks(arg->count,
                        [](const vx_task_t& t, tex_kat_arg_t* a) { kernel_body(t, a); }, arg);
}
