from vstyler.camera import camera_coordinates as generate_camera_coordinates  # noqa: F401
from vstyler.models import AdapterResidualBlock as ResidualBlock, SimpleAdapter  # noqa: F401
