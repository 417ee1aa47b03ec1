// host_threads.h (internal) -- the helper threads of HPRIOffline<GPU>::process (hps.cpp): a thread that is always joined,
// the prefaulter of a vector's reserved pages, and the owner of the thread that frees a by-value clip.  Not part of the
// installed interface under libzen/libzen/.
#ifndef ZG_HOST_THREADS_H
#define ZG_HOST_THREADS_H

#include <cstddef>
#include <cstdint>
#include <exception>
#include <mutex>
#include <optional>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

#include <sys/mman.h>

#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif

namespace zen {
namespace internal {
	namespace host {
	namespace { // internal linkage: hps.cpp is the one translation unit that includes this, and libzen.so exports none of it

		// f() on a thread of its own, joined by the destructor at the latest.  Where the system starts no thread, f is kept
		// and finish() runs it on the caller's thread: no helper is ever a reason for a call to fail.
		template <typename F>
		class Helper {
		public:
			explicit Helper(F f)
			    : f_(std::move(f))
			{
				try {
					t_ = std::thread([this] {
						try {
							f_();
						}
						catch (...) {
							err_ = std::current_exception();
						}
					});
					started_ = true;
				}
				catch (const std::system_error&) {
				}
			}
			Helper(const Helper&) = delete;
			Helper& operator=(const Helper&) = delete;
			~Helper()
			{
				if (t_.joinable())
					t_.join();
			}

			bool started() const { return started_; }

			// joins and rethrows what f threw; without a thread, f runs here (once)
			void finish()
			{
				if (!started_) {
					started_ = true;
					f_();
				}
				if (t_.joinable())
					t_.join();
				if (err_)
					std::rethrow_exception(std::exchange(err_, nullptr));
			}

		private:
			F f_;
			std::exception_ptr err_;
			bool started_ = false;
			std::thread t_;
		};

		// The whole 4 KB pages of [p, p + bytes) as [a, e); false where they are fewer than 8 huge pages (16 MB), which are
		// not worth a thread.
		inline bool page_span(const void* p, std::size_t bytes, std::uintptr_t& a, std::uintptr_t& e)
		{
			const std::uintptr_t page = 4096, huge = (std::uintptr_t)2 << 20;
			a = ((std::uintptr_t)p + page - 1) & ~(page - 1);
			e = ((std::uintptr_t)p + bytes) & ~(page - 1);
			return e >= a + 8 * huge;
		}

		// The pages of a vector's RESERVED capacity asked for as transparent huge pages and faulted in by helper threads that
		// nobody waits for until the destructor: the vector is filled behind them.  Only advice to the kernel about memory the
		// vector owns; where it is refused, or a helper does not start, whoever writes the pages faults them in.
		class Prefaulter {
		public:
			Prefaulter(void* p, std::size_t bytes)
			{
				std::uintptr_t a, e;
				if (!page_span(p, bytes, a, e))
					return;
				(void)madvise((void*)a, e - a, MADV_HUGEPAGE);
				unsigned k = std::thread::hardware_concurrency() / 8;
				k = k < 1 ? 1 : k > kMax ? kMax : k;
				for (unsigned i = 0; i < k; ++i) {
					th_[i].emplace(Pieces{a, e, i, k});
					if (!th_[i]->started())
						break;
				}
			}

		private:
			static constexpr unsigned kMax = 6;
			// 32 MB pieces dealt round robin, so that the helpers together advance through the vector from its start -- the
			// order in which it is filled
			struct Pieces {
				std::uintptr_t a, e;
				unsigned i, k;
				void operator()() const
				{
					const std::uintptr_t piece = (std::uintptr_t)32 << 20;
					for (std::uintptr_t b0 = a + i * piece; b0 < e; b0 += k * piece)
						(void)madvise((void*)b0, (b0 + piece < e ? piece : e - b0), MADV_POPULATE_WRITE);
				}
			};
			std::optional<Helper<Pieces>> th_[kMax];
		};

		// Returning the pages of a long clip to the system takes 25-60 ms per hour of audio (one munmap of 635 MB): a helper
		// does it while the caller goes on.  One object per process, built on first use (no thread exists before that), at most
		// one thread, joined by the next take() and by the destructor at exit.
		class DeferredFree {
		public:
			static DeferredFree& instance()
			{
				static DeferredFree d;
				return d;
			}
			void take(std::vector<float>&& clip)
			{
				std::lock_guard<std::mutex> lock(m_);
				t_.reset(); // joins the helper of the call before, which has long finished
				t_.emplace(Drop{std::move(clip)});
				if (!t_->started())
					t_.reset(); // no thread: the clip is freed here, on the caller's clock
			}

		private:
			struct Drop {
				std::vector<float> clip;
				void operator()() { std::vector<float>().swap(clip); }
			};
			std::mutex m_;
			std::optional<Helper<Drop>> t_;
		};

	} // namespace
	} // namespace host
} // namespace internal
} // namespace zen

#endif /* ZG_HOST_THREADS_H */
