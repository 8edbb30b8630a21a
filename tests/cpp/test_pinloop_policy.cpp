// test_pinloop_policy.cpp -- the Levenberg-Marquardt policy of the two pinhole loops, pc_next / pc_accepts of
// csrc/mcc_pincalib_internal.h, compiled for the host and driven through a table (tests/test_pinloop_policy.py).
// The device calls the same function from pin_verdict (csrc/mcc_pinloop_device.hpp); every row starts from the
// state `base` with a few fields set, makes one transition and compares every field of the result.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "mcc_pincalib_internal.h"

namespace {

using mcc::PcState;

const double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();

PcState base() {
    PcState s{};
    s.iter = 3;
    s.tries = 2;
    s.trials = 7;
    s.status = -1;   // (no kPc* code: a transition that does not end the loop leaves it alone)
    s.crit_type = 3;
    s.max_count = 30;
    s.eps = 1e-6;
    s.lambda = 1e-4;
    s.err = 50.0;
    s.change = 0.25;
    return s;
}

bool same_double(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }

int check(const char* name, const PcState& got, const PcState& want) {
    const bool ok = got.iter == want.iter && got.tries == want.tries && got.trials == want.trials && got.done == want.done &&
                    got.status == want.status && got.init == want.init && got.relin == want.relin && got.fail == want.fail &&
                    got.crit_type == want.crit_type && got.max_count == want.max_count && same_double(got.eps, want.eps) &&
                    same_double(got.lambda, want.lambda) && same_double(got.err, want.err) &&
                    same_double(got.change, want.change);
    if (!ok)
        std::printf("FAIL %s: iter %d/%d tries %d/%d trials %d/%d done %d/%d status %d/%d init %d/%d relin %d/%d fail %d/%d "
                    "lambda %.17g/%.17g err %.17g/%.17g change %.17g/%.17g\n",
                    name, got.iter, want.iter, got.tries, want.tries, got.trials, want.trials, got.done, want.done, got.status,
                    want.status, got.init, want.init, got.relin, want.relin, got.fail, want.fail, got.lambda, want.lambda,
                    got.err, want.err, got.change, want.change);
    return ok ? 0 : 1;
}

PcState rejected(PcState s) {
    s.trials += 1;
    s.tries += 1;
    s.lambda = s.lambda * 10.0;
    s.relin = 0;
    return s;
}

PcState accepted(PcState s, double en, double change) {
    s.trials += 1;
    s.iter += 1;
    s.tries = 0;
    s.relin = 1;
    s.err = en;
    s.change = change;
    s.lambda = std::fmax(s.lambda * 0.1, 1e-12);
    return s;
}

}  // namespace

int main() {
    int bad = 0, cases = 0;
    auto row = [&](const char* name, const PcState& s, double en, double change, const PcState& want) {
        ++cases;
        bad += check(name, mcc::pc_next(s, en, change), want);
    };

    {   // the start: its error is taken, whatever err held, and the next lin kernel linearises
        PcState s = base(), w;
        s.init = 1;
        s.relin = 0;
        s.err = 0.0;
        w = s;
        w.err = 12.5;
        w.init = 0;
        w.relin = 1;
        row("init finite", s, 12.5, 0.0, w);
        for (const double en : {kInf, kNaN}) {
            w = s;
            w.err = en;
            w.init = 0;
            w.relin = 1;
            w.done = 1;
            w.status = mcc::kPcNotFinite;
            row(en != en ? "init NaN" : "init +inf", s, en, 0.0, w);
        }
    }
    {   // rejections
        PcState s = base();
        s.relin = 1;
        row("reject", s, 50.5, 0.0, rejected(s));
        ++cases;
        if (rejected(s).lambda != 1e-4 * 10.0 || mcc::pc_accepts(s, 50.5)) {
            ++bad;
            std::printf("FAIL reject: lambda or pc_accepts\n");
        }
        s.tries = 9;
        PcState w = rejected(s);
        w.done = 1;
        w.status = mcc::kPcStalled;
        row("tenth rejection in a row", s, 50.5, 0.0, w);
        s = base();
        s.tries = 8;
        row("ninth rejection in a row", s, 50.5, 0.0, rejected(s));
        s = base();
        s.fail = 1;
        row("failed factorisation with en < err", s, 10.0, 1e-9, rejected(s));
        s = base();
        row("en NaN", s, kNaN, 1e-9, rejected(s));
    }
    {   // acceptances
        PcState s = base();
        s.relin = 0;
        row("en == err", s, 50.0, 0.5, accepted(s, 50.0, 0.5));
        row("accept", s, 40.0, 0.5, accepted(s, 40.0, 0.5));
        ++cases;
        if (mcc::pc_next(s, 40.0, 0.5).lambda != 1e-4 * 0.1 || !mcc::pc_accepts(s, 50.0)) {
            ++bad;
            std::printf("FAIL accept: lambda or pc_accepts\n");
        }
        s.lambda = 1e-12;
        PcState w = accepted(s, 40.0, 0.5);
        row("lambda stays at its floor", s, 40.0, 0.5, w);
        ++cases;
        if (w.lambda != 1e-12) {
            ++bad;
            std::printf("FAIL floor: %.17g\n", w.lambda);
        }
    }
    {   // stop tests
        PcState s = base(), w;
        s.crit_type = 2;
        w = accepted(s, 40.0, 1e-7);
        w.done = 1;
        w.status = mcc::kPcConverged;
        row("crit 2, change < eps", s, 40.0, 1e-7, w);
        row("crit 2, change == eps", s, 40.0, 1e-6, accepted(s, 40.0, 1e-6));
        s.iter = 29;
        row("crit 2 ignores the count", s, 40.0, 0.5, accepted(s, 40.0, 0.5));
        s.crit_type = 1;
        w = accepted(s, 40.0, 0.5);
        w.done = 1;
        w.status = mcc::kPcCount;
        row("crit 1, iter + 1 == max_count", s, 40.0, 0.5, w);
        w = accepted(s, 40.0, 1e-7);
        w.done = 1;
        w.status = mcc::kPcCount;
        row("crit 1 ignores eps", s, 40.0, 1e-7, w);
        s.iter = 28;
        row("crit 1, iter + 1 < max_count", s, 40.0, 0.5, accepted(s, 40.0, 0.5));
        s.crit_type = 3;
        s.iter = 29;
        w = accepted(s, 40.0, 1e-7);
        w.done = 1;
        w.status = mcc::kPcConverged;
        row("crit 3, both", s, 40.0, 1e-7, w);
    }
    std::printf("%d cases, %d failed\n", cases, bad);
    if (!bad) std::printf("policy ok\n");
    return bad ? 1 : 0;
}
