"""What the raw-launch SpMM tests share (policy, walk, fused, rows, hub_parts): NaN-filled buffers, the caller-allocated
outputs of one output form, the generic reference route and the word-for-word comparison.  The launches themselves are
recommendation_amd/spmm_launch.py's."""
import torch

from recommendation_amd import spmm_launch as L


def nan(rows, d):
    """[max(rows, 1), d] of NaN on the GPU: a word a launch did not write shows."""
    return torch.full((max(int(rows), 1), d), float("nan"), device="cuda")


class Out:
    """The outputs of one launch for a form (want_y, acc_in: None | 'given' | 'inplace', want_acc, val_scale, acc_scale):
    y and acc_out NaN-filled where wanted, acc_in a copy of the given rows (in place: acc_out is that copy)."""

    def __init__(self, n_rows, d, form, acc_in):
        want_y, a_in, want_acc, self.val_scale, self.acc_scale = form
        self.y = nan(n_rows, d) if want_y else None
        self.acc_out = nan(n_rows, d) if want_acc else None
        self.acc_in = acc_in.clone() if a_in else None
        if a_in == "inplace":
            self.acc_out = self.acc_in

    def kw(self):
        """The form as the keywords every launch function with an epilogue takes."""
        return dict(y=self.y, acc_in=self.acc_in, acc_out=self.acc_out, val_scale=self.val_scale, acc_scale=self.acc_scale)


def generic(csr, plan, x, d, partials, **form):
    """The reference route: `spmm_parts` over `plan` (gcr_spmm_csr_acc2_f32 without mask, second addend or row normalise).
    Rows the plan skips stay as they were."""
    L.csr_acc2(csr, plan, x=x, d=d, partials=partials, acc_in2_scale=0.0, on=x, **form)


def assert_words_equal(got, want, what):
    """Both absent, or every 32-bit word equal."""
    assert (got is None) == (want is None), what
    if got is not None:
        assert got.shape == want.shape, f"{what}: {tuple(got.shape)} against {tuple(want.shape)}"
        differ = got.view(torch.int32) != want.view(torch.int32)
        assert not bool(differ.any()), \
            f"{what}: {int(differ.sum())} of {differ.numel()} words differ, first at {differ.nonzero()[0].tolist()}"
