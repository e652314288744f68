// lgh_timing.hip — what measures the library from inside: the region timers (HIP events around the reference's stopwatch
// regions), the event pairs around single kernels (lgh_ktime_*) and the roctx ranges.
#include <atomic>
#include <dlfcn.h>

#include "lgh_common.hpp"

namespace lgh
{

void timer_start(lgh_ctx *c)
{
   if (!c->timers.enabled) { return; }
   (void)hipEventRecord(c->timers.ev[0], c->stream);
}
void timer_stop(lgh_ctx *c, int which)
{
   if (!c->timers.enabled) { return; }
   (void)hipEventRecord(c->timers.ev[1], c->stream);
   (void)hipEventSynchronize(c->timers.ev[1]);
   float ms = 0.f;
   (void)hipEventElapsedTime(&ms, c->timers.ev[0], c->timers.ev[1]);
   c->timers.t[which] += 1e-3 * ms;
}

// ---- roctx ranges (LGH_ROCTX=1): the library is loaded by the first context created with the switch, for the process
namespace
{
struct Roctx
{
   int (*push)(const char *) = nullptr;
   int (*pop)() = nullptr;
   Roctx()
   {
      void *h = nullptr;
      for (const char *n : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"})
      {
         h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
         if (h) { break; }
      }
      if (!h) { return; }
      push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
      pop = (int (*)())dlsym(h, "roctxRangePop");
      if (!push || !pop) { push = nullptr; pop = nullptr; }
   }
};
std::atomic<const Roctx *> g_roctx{nullptr};
} // namespace
void roctx_enable()
{
   static const Roctx r;
   g_roctx.store(&r);
}
RoctxRange::RoctxRange(const char *name) : on(false)
{
   const Roctx *r = g_roctx.load();
   on = r && r->push != nullptr;
   if (on) { (void)r->push(name); }
}
RoctxRange::~RoctxRange()
{
   if (on) { (void)g_roctx.load()->pop(); }
}

} // namespace lgh

using namespace lgh;

extern "C"
{

int lgh_get_timers(lgh_ctx *c, double t[4], long n[3])
{
   LGH_CHECK_ARG(c && t && n);
   for (int i = 0; i < 4; i++) { t[i] = c->timers.t[i]; }
   for (int i = 0; i < 3; i++) { n[i] = c->timers.c[i]; }
   return LGH_OK;
}
int lgh_reset_timers(lgh_ctx *c)
{
   LGH_CHECK_ARG(c);
   for (int i = 0; i < 4; i++) { c->timers.t[i] = 0; }
   for (int i = 0; i < 3; i++) { c->timers.c[i] = 0; }
   return LGH_OK;
}
int lgh_enable_timers(lgh_ctx *c, int on)
{
   LGH_CHECK_ARG(c);
   c->timers.enabled = on != 0;
   return LGH_OK;
}

int lgh_ktime_begin(lgh_ctx *c, int which, int max_samples)
{
   LGH_CHECK_ARG(c && which >= 0 && max_samples > 0);
   if (!c->ktime) { c->ktime.reset(new KTime()); }
   KTime *k = c->ktime.get();
   while ((int)k->ev.size() < 2 * max_samples)
   {
      hipEvent_t e;
      LGH_HIP_CHECK(hipEventCreate(&e));
      k->ev.push_back(e);
   }
   k->which = which;
   k->max = max_samples;
   k->n = 0;
   return LGH_OK;
}
int lgh_ktime_end(lgh_ctx *c, int *launches, double *mean_seconds)
{
   LGH_CHECK_ARG(c && launches && mean_seconds && c->ktime);
   KTime *k = c->ktime.get();
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   double tot = 0.0;
   for (int i = 0; i < k->n; i++)
   {
      float ms = 0.f;
      LGH_HIP_CHECK(hipEventElapsedTime(&ms, k->ev[2 * i], k->ev[2 * i + 1]));
      tot += 1e-3 * ms;
   }
   *launches = k->n;
   *mean_seconds = k->n ? tot / k->n : 0.0;
   k->which = -1;
   return LGH_OK;
}

} // extern "C"
