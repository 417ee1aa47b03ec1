/* libzen_hip_fake.so for tests/test_addon_binding.py: the calls zen_amd/_addon.py's Handle makes, counted; no device */
typedef struct { unsigned long long created, destroyed, streams; int profiling; } zen_hip_fake_stats_t;
static zen_hip_fake_stats_t st;
static const char *msg = "";
static int fail(int rc, const char *m) { msg = m; return rc; }
const char *zen_hip_fake_last_error(void) { return msg; }
int zen_hip_fake_fail(int rc) { return fail(rc, "fake_fail: as asked"); }
int zen_hip_fake_create(int rc, void **h) { if (rc) return fail(rc, "fake_create: refused"); *h = &st; ++st.created; return 0; }
int zen_hip_fake_destroy(void *h) { (void)h; ++st.destroyed; return 0; }
int zen_hip_fake_set_stream(void *h, void *s) { (void)s; if (!h) return fail(2, "fake_set_stream: null handle"); ++st.streams; return 0; }
int zen_hip_fake_stats(void *h, zen_hip_fake_stats_t *out) { (void)h; *out = st; return 0; }
int zen_hip_fake_profile(void *h, int on) { (void)h; st.profiling = on; return 0; }
int zen_hip_fake_profile_get(void *h, double *ms, unsigned long long *bytes, unsigned long long *launches) {
	for (int k = 0; k < 3; ++k) { ms[k] = 0.5 + k; bytes[k] = 100ull * (k + 1); launches[k] = k + 1; }
	return h ? 0 : fail(2, "fake_profile_get: null argument");
}
