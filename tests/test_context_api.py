"""generate(context=...) / encode_context argument checks: everything that is refused is refused before any encode, so these run without a
GPU (the GPU side is tests/test_hip_prefix.py)."""
from __future__ import annotations

from types import SimpleNamespace

import pytest
import torch


def _model(name="tiny"):
    from eilev_amd.configs import blip2_config
    from eilev_amd.model.v2 import VideoBlipForConditionalGeneration

    return VideoBlipForConditionalGeneration(blip2_config(name))


def _context(P=10):
    """A context as encode_context makes it, without the engine behind it: the checks under test only read its length."""
    from eilev_amd.model.v2 import VideoContext

    return VideoContext(SimpleNamespace(P=P), torch.ones(1, P, dtype=torch.long), key=None)


def test_every_unsupported_combination_is_named():
    from transformers import LogitsProcessorList, MaxLengthCriteria, MinLengthLogitsProcessor, StoppingCriteriaList

    m, ctx = _model(), _context()
    one = torch.ones(1, 4, dtype=torch.long)
    refused = [
        ("num_beams", dict(num_beams=3)),
        ("do_sample", dict(do_sample=True)),
        ("logits processors", dict(repetition_penalty=1.3)),
        ("logits processors", dict(no_repeat_ngram_size=2)),
        ("logits processors", dict(logits_processor=LogitsProcessorList([MinLengthLogitsProcessor(2, 1)]))),
        ("stopping criteria", dict(stopping_criteria=StoppingCriteriaList([MaxLengthCriteria(8)]))),
        ("stopping criteria", dict(max_time=1.0)),
        ("several EOS ids", dict(eos_token_id=[2, 5])),
        ("min_new_tokens", dict(min_new_tokens=2)),
        ("min_new_tokens", dict(min_new_tokens=4)),  # (= max_new_tokens: the plain route folds this into "no EOS"; here it is still named)
        ("output_scores", dict(return_dict_in_generate=True, output_scores=True)),
        ("output_scores", dict(return_dict_in_generate=True, output_logits=True)),
        ("prompt_lookup_num_tokens", dict(prompt_lookup_num_tokens=3)),
    ]
    for name, kw in refused:
        with pytest.raises(NotImplementedError, match=name) as e:
            m.generate(one, max_new_tokens=4, context=ctx, **kw)
        assert "context" in str(e.value), name
    with pytest.raises(NotImplementedError, match="num_beams > 1, do_sample=True"):
        m.generate(one, max_new_tokens=4, context=ctx, num_beams=2, do_sample=True)
    with pytest.raises(TypeError, match="encode_context"):
        m.generate(one, max_new_tokens=4, context=object())


def test_the_length_check_counts_the_context():
    m = _model()
    limit = m.config.text_config.max_position_embeddings
    one = torch.ones(1, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        m.generate(one, max_new_tokens=limit - 10 - 4 + 1, context=_context(10))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        m.generate(one, max_length=limit + 1, context=_context(10))  # max_length counts P + S
    with pytest.raises(ValueError, match="max_position_embeddings"):
        m.generate(one, max_new_tokens=2, context=_context(limit - 5))
    # inside the limit the call passes every check and reaches the engine, which needs a GPU (no CPU fallback)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            m.generate(one, max_new_tokens=limit - 10 - 4, context=_context(10))
    with pytest.raises(ValueError, match=r"\(1, P\)"):
        m.encode_context(torch.ones(2, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        m.encode_context(torch.ones(1, limit, dtype=torch.long))


def test_flan_t5_has_no_context():
    from eilev_amd.configs import CONFIGS

    name = next(n for n, c in CONFIGS.items() if c["text_config"].get("model_type") == "t5")
    m = _model(name)
    one = torch.ones(1, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="flan-t5"):
        m.encode_context(one)
    with pytest.raises(NotImplementedError, match="flan-t5"):
        m.generate(one, max_new_tokens=2, context=_context())


def test_classify_passes_share_prompt_cache_on():
    import inspect

    from eilev_amd.engine import HipEngine
    from eilev_amd.model.v2 import VideoBlipForConditionalGeneration

    for fn in (VideoBlipForConditionalGeneration.classify, HipEngine.classify_loglik):
        assert inspect.signature(fn).parameters["share_prompt_cache"].default is False
