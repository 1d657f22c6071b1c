from .encoder_decoder import EncoderDecoder  # noqa: F401
from .dynamic_encoder_decoder import DynamicEncoderDecoder  # noqa: F401
from .dynamic_distiller import DynamicDistiller  # noqa: F401
from .cascade_encoder_decoder import CascadeEncoderDecoder, DynamicCascadeEncoderDecoder  # noqa: F401
