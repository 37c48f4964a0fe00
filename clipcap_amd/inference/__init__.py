"""clipcap_amd.inference — decoding entry points (reference clipcap/inference/)."""
from clipcap_amd.inference.base import generate_beam, generate_beam_tokens, generate_no_beam, generate_nucleus_sampling  # noqa: F401
from clipcap_amd.inference.contrastive import generate_contrastive, generate_contrastive_tokens  # noqa: F401
from clipcap_amd.inference.generate import generate  # noqa: F401
from clipcap_amd.inference.lexical import (ConstrainedBeams, best_constrained_beams, generate_constrained_beam,  # noqa: F401
                                           generate_constrained_beam_tokens)
from clipcap_amd.inference.score import CaptionScores, rerank_captions, score_captions  # noqa: F401
from clipcap_amd.inference.stochastic_beam import (StochasticBeams, generate_stochastic_beam, generate_stochastic_beam_tokens,  # noqa: F401
                                                   sbs_importance_weights)
